/*
 * evo_amd.h -- C ABI of libevo_amd.so: the MI355X (gfx950) implementation of the EVO
 * evolutionary-variational E-step / M-step hot path (EBSC and ES3C).
 *
 * The reference (tvlearn/evo) has no FFI: its "operator API" is the Python method set of
 * evo.models.Model / evo.variational.* operating on three dicts of NumPy arrays
 * (SURVEY.md 8b).  This header is what the reference-side binding (a ctypes stub inside
 * evo/models/{_models,bsc,sssc}.py, shown in INTEGRATION.md) binds; evo_amd/_lib.py is
 * that stub for our own host-side mirror.  Each entry point names the reference lines it
 * replaces (paths relative to the reference root).
 *
 * Conventions: plain C, no exceptions.  Every function returns 0 on success and a
 * negative EVOAMD_E_* code on failure; evoamd_last_error() then returns a message.
 * Host pointers are borrowed for the duration of the call only.  Device work is ordered on
 * the context's stream; every call that returns data to the host (download_*, lpj_* with an
 * output pointer, vary_kn with sums_out, stats, free_energy) has completed it on return, the
 * others (lpj_resident, evolve_randflip, set_params_*) may return while kernels are still
 * queued, and device-side error conditions (EVOAMD_E_KLIMIT / _SINGULAR) are reported by the
 * next host-returning call.  One context per GPU per process; a context is not thread-safe.  All floating point is IEEE binary64 (the reference is float64-only).
 *
 * State encoding on the device: a binary state s in {0,1}^H is HW = ceil(H/64) 64-bit
 * words; latent h lives in word h/64 at bit 63-(h%64) (MSB first), so that comparing the
 * words as unsigned integers, word 0 first, is the lexicographic order np.unique applies
 * to the reference's int rows (evo/variational/utils.py:279-282).  Host-facing calls take
 * the reference's own layout: C-contiguous bool (1 byte per latent).
 */
#ifndef EVO_AMD_H
#define EVO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVOAMD_ABI_VERSION 1

enum {
  EVOAMD_OK = 0,
  EVOAMD_E_INVALID = -1, /* bad argument / call order                               */
  EVOAMD_E_HIP = -2,     /* a HIP runtime call failed (message has the HIP error)    */
  EVOAMD_E_NODEVICE = -3,/* no gfx950 device visible                                 */
  EVOAMD_E_RCCL = -4,    /* RCCL missing or a collective failed                      */
  EVOAMD_E_KLIMIT = -5,  /* ES3C, fused E-step kernel only: more than EVOAMD_KCAP active latents (the separate passes solve such a state in global memory) */
  EVOAMD_E_SINGULAR = -6 /* ES3C: exactly singular k x k system (reference: pinv path)*/
};

enum { EVOAMD_MODEL_BSC = 0, EVOAMD_MODEL_SSSC = 1 };

/* ES3C: largest |s| whose k x k system the wavefront kernel holds in LDS (one wavefront per state); a state with more
 * active latents is solved by the same kernel in global memory (slots allocated by evoamd_configure when H > 64). */
#define EVOAMD_KCAP 64

typedef struct evoamd_ctx evoamd_ctx;

/* ---- library / context ------------------------------------------------------------- */
int evoamd_abi_version(void);
const char *evoamd_last_error(void);
int evoamd_device_count(int *count);
/* Creates a context on HIP device `device` (one non-default stream, workspace allocated
 * lazily by evoamd_configure). */
int evoamd_ctx_create(int device, evoamd_ctx **out);
void evoamd_ctx_destroy(evoamd_ctx *ctx);
int evoamd_synchronize(evoamd_ctx *ctx);
/* Debug aid: process-wide counts of live device (out[0]) and pinned host (out[1]) allocations of the library.  Equal
 * before a context is created and after it is destroyed: no buffer outlives its context. */
int evoamd_debug_live_buffers(int64_t out[2]);
/* Debug aid: the host-side validity state of a context (DESIGN: what a change invalidates).  out[0] = the boolean fields
 * at the bit positions below, then gen, kn_gen, theta_gen, pending_skip, census_skip, kn_refill, pred_N.  Reads host
 * fields only: no HIP call, no synchronisation. */
enum {
  EVOAMD_VB_HAVE_DATA = 0, EVOAMD_VB_HAVE_PARAMS = 1, EVOAMD_VB_HAVE_CAND = 2, EVOAMD_VB_B_VALID = 3,
  EVOAMD_VB_ROWS_FRESH = 4, EVOAMD_VB_STATS_ROWS_VALID = 5, EVOAMD_VB_YHAT_VALID = 6, EVOAMD_VB_REC_RESIDENT = 7,
  EVOAMD_VB_YREC_VALID = 8, EVOAMD_VB_YREC_FROM_PASS = 9, EVOAMD_VB_REC_IN_STATS = 10, EVOAMD_VB_KEEP_X_VALID = 11,
  EVOAMD_VB_REC_USES_KEEP = 12, EVOAMD_VB_NEED_KNOWN = 13, EVOAMD_VB_RES_NEED0 = 14, EVOAMD_VB_RES_NEED1 = 15,
  EVOAMD_VB_RES_NEED2 = 16, EVOAMD_VB_CAND_FROM_DEVICE = 17, EVOAMD_VB_LISTS_CLEAN = 18, EVOAMD_VB_CLIST_CLEAN = 19,
  EVOAMD_VB_ACC_CLEAN = 20, EVOAMD_VB_WQ_COPY_VALID = 21, EVOAMD_VB_H_THETA_FRESH = 22, EVOAMD_VB_THETA_BAK_VALID = 23,
  EVOAMD_VB_KN_LOST = 24, EVOAMD_VB_LAST_ESTEP_FUSED = 25, EVOAMD_VB_REDUCE_PENDING = 26, EVOAMD_VB_BINS_DIRTY = 27,
  EVOAMD_VB_GEN_KEPT = 28,          /* gen_keep >= 0: an evoamd_generate call has completed */
  EVOAMD_VB_PREFETCH_CURRENT = 29,  /* prefetch_gen == gen */
  EVOAMD_VB_CENSUS_CURRENT = 30,    /* census_gen == kn_gen */
  EVOAMD_VB_ROWS_KN_CURRENT = 31    /* rows_kn_gen == kn_gen */
};
int evoamd_debug_validity(evoamd_ctx *ctx, int64_t out[8]);
/* Options: "ebsc_f32" (0/1, default 0; read by the next evoamd_configure of an EBSC geometry): float32 mode -- the data,
 * B = Y W and the per-datapoint E_q[s] rows are stored in float and the two long contractions (B = Y W, Wp = Es^T Y) run
 * on v_mfma_f32_16x16x4_f32; lpj arithmetic, selection, every accumulator and Theta stay float64 (the reference has no
 * float32 at all: BASELINE.json configs[4] asks for it).  Parity with the float64 path: lpj / F to ~1e-6 relative,
 * Theta to ~1e-5, K^n not bit-identical.  No incomplete data, reconstruction or bsc_direct in this mode.
 * "bsc_direct" (0/1, default 0): evaluate EBSC batches with the direct residual kernel
 * (the reference's arithmetic, bsc.py:91-93) instead of the Gram-form kernel.  Takes effect at the
 * next evoamd_set_params_bsc.  "sssc_k8" (1 / 0 / -1, default -1): serve ES3C states with 5..8 active
 * latents with the K=8 register kernel / the LDS wavefront kernel / whichever the counts of the last
 * statistics pass favour.  "state_digest" (0/1, default 1): the lpj and statistics kernels read the
 * 8-byte per-state digests (count + first four active latents, maintained by every kernel that
 * writes states) instead of the ceil(H/64) bit words; 0 selects the word path (A/B, tests).
 * "overlap_gemm" (0 / 1 / 2, default 1): evoamd_mstep_device runs the K = N statistics contraction on a
 * second stream beside the H x H elimination chain (single rank, no kernel timing; neither reads what
 * the other writes): never / for the shapes where it was measured to pay (ES3C, large H) / always.
 * "inverse_spd" (0/1, default 1): the H x H inverses of the device Theta update by the SPD block
 * Gauss-Jordan (diagonal blocks as pivots; a bad pivot reports status 3 and the update is repeated with
 * partial pivoting) / always the partially pivoted elimination.  "reconstruct_in_stats" (one-shot): the
 * next statistics pass forms y_reconstructed between the moment rows and the Wp contraction
 * (bsc.py:184-189, sssc.py:630-633).
 * "inverse_block" (0 / 16 / 32, default 0): columns eliminated per launch by the SPD block Gauss-Jordan;
 * 0 = up to n = 128 the whole elimination in ONE launch (one workgroup per matrix, the matrix in its registers), 32 from
 * n = 256 on (32 x 32 pivot block inverted in registers through its Schur complement), 16 in between; 16 / 32 force the
 * multi-launch forms.
 * "merge_select_fused" (0/1, default 0): evoamd_patches_merge_resident writes y_rec as N x D rows first and merges those
 *   (0, measured faster) or selects while it gathers (1); same image bit for bit, see there.
 * "prefetch_lpj" (0/1, default 1): evoamd_mstep_device enqueues the next iteration's evoamd_lpj_resident
 * pass behind its mailbox kernel (the GPU works while the host turns the iteration around); the next
 * evoamd_lpj_resident call returns at once unless Theta, K^n, the data or an option changed in between.
 * "stats_chunks" (1 .. 16, default 1; measured slower than one block at the north-star shape, kept for A/B): the statistics pass of large shards (contraction >= 8 GFLOP) runs in that many
 * blocks of datapoints; the MFMA contraction of block i runs on the second stream beside the scatter kernels of block
 * i + 1 (those are bound by the f64 atomic rate, the contraction by the matrix cores); 1 = one block.  "overlap_gemm" = 0
 * switches this off as well.  "pair_bins" (0 / 1 / 2, default 1): the ES3C statistics pass appends the second-moment
 * contributions of the states with two active latents to row bins and reduces each bin in an LDS tile instead of
 * issuing two global f64 atomics per state: never / when the tiles' flush is a small part of the contributions
 * (large N S) / always.  "stats_stage" (0/1, default 1): that kernel stages the B row of each datapoint and the singleton table
 * in LDS when two workgroups per CU still fit.  "stats_waves" (0 / 8 / 16, measurement aid): waves per workgroup of the
 * ES3C statistics kernel (0 = 4).  "gemm_streamk" (0/1, default 1): the long-K 128-tile contraction runs as ONE resident-sized grid -- every XCD owns an eighth
 * of K, its workgroups cut the (tile, K slab) units of that range into equal runs -- instead of tiles x 64 K chunks.
 * "b_transposed" (0/1/2, default 1; read by the next evoamd_configure): from N = 8192 datapoints, H = 768 and D = 128 on
 * (2: from H = 128, D = 32 on) the context keeps Y^T as well and computes B = Y W with the 128 x 128 tile kernel; 0: always
 * the row-major 64 x 64 tile product.
 * "pair_bins_scale" (1 .. 64, default 3; read by the next evoamd_configure): entry capacity of the pair bins in units of
 * N x S entries of 32 bytes (a K^n of mostly 5..8 active latents needs ~12; entries beyond the capacity fall back to atomics).
 * "pair_bins_nwg" (256 .. 2048 in steps of 256, default 2048; read by the next evoamd_configure): producer workgroups of
 * the statistics pass = private regions per pair bin (fewer, longer regions for the reduce pass to read).
 * "pair_bins_auto" (0/1, default 1): the statistics pass re-cuts the pair bins (grows "pair_bins_scale", up to 64) when the
 * census of the previous pass -- states with 3..4 / 5..8 active latents leave up to 6 / 28 entries each -- says the K^n has
 * outgrown them, instead of overflowing onto the atomic fallback; 0: the configured capacity stays.
 * "pair_bins_min" (default 256): with "pair_bins" = 1 the bins are used from this many x 1024 resident states (N S) on.
 * "bsc_stats_wave" (0/1, default 1): EBSC statistics on the wave-per-datapoint kernel (next datapoint prefetched, Wq pairs
 * through the pair bins, column sums in the kernel); 0: the one-shot kernel + column-sum pass.
 * "gemm_workspace" (0/1, default 1): the stream-K workgroups store their partial tiles to a workspace and a second kernel
 * adds them to C in a fixed order; 0: they add to C with f64 atomics (all of them at once, when the runs end).
 * "sssc_precision" (64 / 32, default 64): SSSC(precision=np.float32) of the reference (evo/models/sssc.py:49, 344-349,
 * 484-498): 1 / sigma2 and D log sigma2 pass through float32 and the moment sums (xpt_s, xpt_ss, xpt_sz, xpt_szsz,
 * s_sz_outer, sz_sz_outer) are float32 VALUES; every product and sum is still formed in double on the device and rounded
 * once (the reference accumulates them in float32 arrays datapoint by datapoint).
 * "lpj_main_unstaged" (0/1, default 1): ES3C batches whose B rows do not fit the LDS of the table-driven lpj kernel (candidate
 * batches: 1024 / Cmax datapoints per workgroup) run on that kernel with the B values gathered from global memory; 0: on the
 * K = 2 register kernel, which eliminates a 2 x 2 system per state.
 * "lpj_singular_screen" (0 / 1 / 2, default 1): ES3C states with three or more active latents whose Psi_A is exactly
 * singular, the reference's way (evo/models/sssc.py:278-301: pinv(Psi_s), slogdet = -inf, lpj = +inf -> B_max, Lam =
 * inv(G_A / sigma2 + pinv(Psi_A)), pinv of that if it is exactly singular too).  The Gram form of the kernels stays regular
 * there (it returns the continuous limit), so telling the cases apart takes an LU of Psi_A per state: in "exact mode" the
 * register / quad kernels pass every such state on to the pivoting wavefront kernel, which screens Psi_A in LAPACK's
 * elimination order and follows the pinv branches (one-sided Jacobi).  1: exact mode for a Theta in which the tables kernel
 * has found an exactly singular 1 x 1 or 2 x 2 principal block of Psi (a dead or a duplicated latent); 2: always (slow:
 * every state above two latents on the wavefront kernel); 0: never.  States with at most two active latents always follow
 * the reference (state-term tables).
 * "gemm_grouped" (0/1, default 1): long-K contractions whose real tiles fill the resident grid with whole K chunks
 * (>= 93 % of the slots) run as a grouped split-K -- the workgroups of one K chunk, one per tile, sit in one XCD and share
 * every slab of the operands through its L2 (a quarter of the stream-K form's HBM reads); 0: always stream-K.
 * "gemm_per_xcd" (0 = automatic): K chunks per XCD of the long-K 128-tile contraction
 * (measurement aid: tools/gemm_sweep.sh).
 * "background_unit" (0/1, default 0): permanent["background"] of the reference (variational/utils.py:42-47) -- the last latent
 * is on in every state: the device evolutionary operators mutate the other H - 1 latents only (eas.py:213-239) and the
 * device Theta update pins its prior to 1 - 1.1e-5 (bsc.py:259-260, sssc.py:718-719).  The host classes set it from
 * my_suff_stat["permanent"].
 * "fold_clear" (0/1, default 1): the selection kernel (evoamd_vary_kn) zeroes the accumulators of the statistics pass that
 * follows and checks + clears the counters of the census lists on its way; 0: a memset and a one-workgroup kernel do.
 * "early_fork" (-1 = automatic, 0, 1): the stream of the forked K = N contraction branches off as soon as the [Es | Ez] rows are
 * written, i.e. in front of the pair-bin reduce and the finish kernel instead of behind them; automatic = for products below
 * 2e10 flops, where it also makes the fork itself pay from 5e8 flops on (c2: 0.377 -> 0.368 ms per iteration).
 * "merge_small_levels" (0/1, default 1): ES3C with census lists / quad kernels -- while the census of the last statistics
 * pass found few states above four active latents (expected <= 256 in the pass at hand), the pivoting wavefront kernel,
 * which runs behind the 3..4 level anyway, serves the 5..8 list as well instead of a launch of its own (a dependent launch
 * costs 10-20 us however little it does: c2 0.385 -> 0.34 ms per iteration).  Same values to ~1e-13; 0: always the
 * four-lanes-per-state kernel for 5..8 latents (what the fused E-step kernel does: bit-for-bit comparisons use 0).
 * "stats_flat" (0/1, default 0: measured a few per cent at N = 100k, a loss at N / 8): with census lists, the ES3C statistics of the states with at most two active latents run
 * on the thread-per-state kernel (1024-thread workgroups owning floor(1024 / S) datapoints per round, 16 waves per CU);
 * 0: the wave-per-datapoint kernel.
 * "stats_kappa" (0/1/2, default 1 = from "stats_kappa_min" x 1024 resident states on, 2 = wherever the shape allows it; the
 * record buffers are allocated by evoamd_configure where the setting asks for the route): ES3C with census lists,
 * digests, complete data, f64 and even H -- the table-driven lpj kernels leave {kappa_0, kappa_1} of every state with at
 * most two active latents beside its lpj (16 bytes per state), evoamd_vary_kn moves an accepted candidate's record with
 * it, and the statistics pass reads the records instead of the B rows and the state-term tables; the Lam terms of the
 * second moments are added once per active set by the finish kernels.  The records count only while they were written
 * under the current Theta for the current K^n (any other change of either drops them and the pass takes the table route
 * unchanged); 0: never written, never read.  EVOAMD_K_STATS_KAPPA counts the passes that took the route.
 * "stats_kappa_min" (default 16384): the automatic setting of "stats_kappa" takes the route from this many x 1024 resident
 * states (N x S) on -- measured on MI355X: 20 M states gain 0.07 ms per EM iteration, 10 M are even, 2.5 M and 0.64 M lose ~0.01.
 * "theta_copy_engine" (0/1, default 0; measured without gain): evoamd_mstep_device downloads Theta^new with asynchronous copies on a third
 * stream (copy engine) beside the kernels queued behind the update; 0: the mailbox kernel writes Theta into the pinned
 * host buffer itself, in front of them.
 * "census_lists" (0/1, default 1; read by the next evoamd_configure): ES3C on complete data with digests -- the resident
 * states with 3..4 / 5..8 / more than 8 active latents are listed by one pass over the digests per K^n (shared by the
 * statistics pass and the next pass over K^n) and served by the four-lanes-per-state kernels; 0: the round-2 chains
 * (lists appended by the main kernels, K = 4 / K = 8 register kernels, wavefront kernel).
 * "sk_spare" (-1 = automatic (default), 0 .. 32): workgroups per XCD that the long-K contraction does not launch while it
 * runs on the second stream beside the H x H elimination chain of the Theta update, so that the chain's kernels find free
 * CU slots (automatic: 4 where the product takes at least three times as long as the chain, else 8).
 * "mailbox_side_stream" (0/1, default 1): the kernel that hands an iteration's scalars (and Theta^new) to the host runs on a
 * side stream beside the refresh of the tables and the prefetched pass instead of in front of them.
 * "fused_estep" (0 / 1 / 2, default 0): evoamd_estep runs the fused wave-per-datapoint kernel never / when the census of the
 * last statistics pass says K^n is sparse (states above four latents in at most a quarter of the datapoints) / whenever the
 * shape allows it.  Same results bit for bit; default off because the separate passes are faster on MI355X at every BASELINE
 * shape (the chain is bound by vector-instruction issue and per-wave latency, not by the HBM bytes fusion saves: DESIGN 3).
 * "debug_poison_list" (one-shot, tests): the next census of the resident K^n gets an out-of-range entry.  Every list entry
 * and every latent index that crosses LDS is range-checked before it becomes an address, so the pass that reads the entry
 * ends in EVOAMD_E_INVALID ("... out of range") instead of a memory fault; the census is rebuilt afterwards.
 * "debug_fail_stats" (one-shot, tests): the next statistics pass, if it is an ES3C pass on complete data, returns
 * EVOAMD_E_INVALID right after its main kernel, between the producers that append to the pair bins and the reduce that
 * clears their counters; the next pass must start from clean bins.  Any statistics pass consumes the option. */
int evoamd_set_option(evoamd_ctx *ctx, const char *name, int value);

/* ---- problem geometry -------------------------------------------------------------- */
/* Allocates device storage for N datapoints on this rank: Y (N,D), K^n (N,S,HW) packed,
 * lpj (N,S_perm+S), candidate batch (N,Cmax,HW) + lpj, parameters and accumulators.
 * S_perm is 0 or 1 (permanent all-zero state; evo/variational/utils.py:39-54).
 * Replaces the array allocation of _init_lpj_and_state_arrays (variational/utils.py:94-95).
 * A call that fails leaves the context unconfigured: every later call answers "configure first" until one succeeds. */
int evoamd_configure(evoamd_ctx *ctx, int model, int64_t N, int D, int H, int S, int S_perm,
                     int Cmax);

/* my_data["y"] (N,D) float64.  Missing entries may hold NaN: evoamd_upload_masks (below) then tells the library
 * which entries are reliable (my_data["x_infr"]) and zeroes the others in the device copy. */
int evoamd_upload_data(evoamd_ctx *ctx, const double *Y);
/* my_suff_stat["ss"] (N,S,H) bool <-> device K^n (bit-packed on the device). */
int evoamd_upload_states(evoamd_ctx *ctx, const uint8_t *ss_bool);
int evoamd_download_states(evoamd_ctx *ctx, uint8_t *ss_bool);
/* The same K^n, bit-packed on the host side too: rows [n0, n0 + n) as np.packbits(ss, axis=-1) lays them out
 * ((n, S, ceil(H/8)) bytes, latent h in byte h/8 at bit 7-(h%8)).  For shards whose bool form
 * (variational/utils.py:95: 1 byte per latent, 10 GB at N=100k S=200 H=512) should not exist on the host;
 * any row range, so a large K^n can be handed over in chunks. */
int evoamd_upload_states_packed(evoamd_ctx *ctx, const uint8_t *packed, int64_t n0, int64_t n);
int evoamd_download_states_packed(evoamd_ctx *ctx, uint8_t *packed, int64_t n0, int64_t n);
/* K^n(0) drawn where it lives: the law of init_states (variational/utils.py:100-138) -- per datapoint rounds of S
 * candidate states with independent bits Bernoulli(p_init) over the varying latents (p_init <= 0: 1 / H), candidates equal
 * to the permanent all-zero state (S_perm = 1) dropped, first occurrences appended in ascending lexicographic row order
 * (np.unique's) behind what is held, until S states are held; with option "background_unit" the last latent is on in every
 * state and is not drawn.  The stream is counter-based, not NumPy's: the bit of (datapoint n, round r, candidate s,
 * latent h) is rng_u01(seed, n, INIT_PURPOSE + r, s * Hv + h) < p_init (csrc/kernels_init.hpp has the definition;
 * evo_amd.variational.init_states_counter is its NumPy mirror, bit for bit).  The reference loops without bound; here a
 * datapoint that is not complete after max_rounds (1 .. 65536; 256 is ample unless S approaches 2^Hv, and such shapes
 * belong to the host function) makes the call return EVOAMD_E_INVALID naming the cap: K^n then counts as not uploaded --
 * every call that reads it refuses until evoamd_upload_states, evoamd_upload_states_packed calls that cover rows 0 .. N-1 in
 * ascending order, a successful evoamd_init_states or a new evoamd_configure.
 * Exact E-steps (S == 2^Hv): table_packed holds the (S, ceil(H/8)) np.packbits rows of the state table as the host function
 * builds it (without the all-zero row when S_perm = 1, with the background unit's bit set); every datapoint gets it and
 * no random number is drawn (refused unless S + S_perm == 2^Hv, Hv < 12; the rows themselves are the caller's).
 * table_packed == NULL: the sampler.
 * Needs evoamd_configure; reads S_perm and "background_unit" from the context.  Like evoamd_upload_states_packed it writes the
 * digests too, and the lpj rows on the device no longer belong to K^n afterwards.  Option "init_states_home" (-1 automatic
 * (default), 0, 1): a wavefront keeps the round's candidates and the held set in LDS / in a slot of global memory
 * (automatic: LDS whenever 16 S (ceil(H/64) + 1) bytes fit one wavefront's share); same results, for tests. */
int evoamd_init_states(evoamd_ctx *ctx, double p_init, uint64_t seed, int max_rounds, const uint8_t *table_packed);
/* K^n seeded from Theta and the data: greedy forward selection on the model's own lpj (csrc/kernels_seed.hpp has the
 * law; evo_amd.variational.seed_states_host is its NumPy mirror).  Deterministic, no random numbers.  Per datapoint,
 * max_active = A steps with quotas q_t = S / A + (t <= S mod A): step t scores every latent j outside the active set
 * A_{t-1} with lpj(A_{t-1} + {j}) -- what evoamd_lpj_resident computes before its clamp, without ljc; not finite, or an
 * ES3C determinant that is not positive: -inf -- ranks them by descending score (ties and -inf: ascending j), writes the
 * q_t best states to the next q_t slots in rank order and keeps the best as A_t.  The S varying slots are filled
 * step-major with S distinct states of sizes 1 .. A; the permanent all-zero state of S_perm = 1 keeps its own column.
 * path_out (N, A): the latent added at each step; lpj_out (N, A): the winner's score; either may be NULL.
 * Refused with EVOAMD_E_INVALID before anything is written (K^n and its validity stay as they were): no Theta installed
 * or no data, incomplete data (masks present), option "background_unit", "ebsc_f32", "bsc_direct" (there is no G),
 * max_active < 1, > S, > H, > 8 (ES3C) or > 64 (EBSC), a quota q_t > H - (t - 1), or an H whose scores do not fit one
 * wavefront's share of LDS (16 H bytes; about H = 9000).  Incomplete data needs evoamd_seed_states_ex; the background unit
 * is out of scope.
 * Like evoamd_init_states it writes the digests too; a prefetched pass, the census and the statistics rows are dropped
 * and the lpj rows on the device no longer belong to K^n afterwards. */
int evoamd_seed_states(evoamd_ctx *ctx, int max_active, int32_t *path_out, double *lpj_out);
/* evoamd_seed_states with flags (0: exactly evoamd_seed_states, every refusal and its text included).
 * EVOAMD_SEED_INCOMPLETE permits incomplete data; it is a permission, not a mode: with masks resident
 * (evoamd_upload_masks) the same law runs with the Gram quantities of the datapoint's reliable entries o = x_infr[n] --
 * G(n) = W_o^T W_o formed per datapoint from W and the resident mask, B_n = y_o^T W_o and |y_o|^2 as evoamd_upload_masks
 * left them (it zeroes the missing entries of Y); Psi, mu, pil_bar, sigma2 and pre1 are not masked -- the lpj that
 * evoamd_lpj_resident computes on masked data.  A datapoint without a reliable entry is scored by the prior alone (EBSC:
 * all equal, so the slots fill in ascending j).  Without masks the complete kernel runs, unchanged.  Refused as above with
 * the flag too: "background_unit", "ebsc_f32", "bsc_direct", a bad max_active or quota, an unknown flag, and scores plus the
 * staged column of W (16 H + 12 D bytes) that do not fit one wavefront's share of LDS.  ES3C keeps max_active rows of
 * G(n) per wavefront: in LDS while 8 max_active ceil64(H) more bytes fit, else in a buffer of the context grown on demand.
 * No atomics, a fixed summation order: two calls give the same bits. */
#define EVOAMD_SEED_INCOMPLETE 1u
int evoamd_seed_states_ex(evoamd_ctx *ctx, int max_active, unsigned flags, int32_t *path_out, double *lpj_out);
/* K^n seeded by a BEAM of partial states (csrc/kernels_seed_beam.hpp has the law; evo_amd.variational.seed_states_beam_host
 * is its NumPy mirror): the law of evoamd_seed_states with the `beam` = B best partial states kept per step and all of them
 * expanded.  Step t scores P_r + {j} for every beam member P_r (rank order) and every j outside it, in the Gram form of
 * evoamd_seed_states and the arithmetic of the member's own path; a set that an earlier member reaches as well is absent (an
 * exact test on the packed words); all candidates are ranked by descending score (ties: ascending parent rank, then ascending
 * j; -inf last), the q_t best go to the next q_t slots in rank order and the first B of them are the next beam.  beam = 1 is
 * evoamd_seed_states bit for bit.  The S states are distinct, step t's have t latents, none is all-zero.
 * path_out (N, A): the path of the rank-0 state of the last step; lpj_out (N, A): the rank-0 score of each step; either may
 * be NULL.  Complete data only.  Refused with EVOAMD_E_INVALID before anything is written, K^n and its validity left as they
 * were: everything evoamd_seed_states refuses (same texts), masks resident, beam < 1, beam > S / max_active (every beam
 * member is a stored state), beam > 16 (SEED_BEAM_MAX), and an (H, beam) whose keys and beams do not fit one wavefront's
 * share of LDS.  No atomics, a fixed summation order: two calls give the same bits.  Timed under EVOAMD_K_SEED_STATES. */
int evoamd_seed_states_beam(evoamd_ctx *ctx, int max_active, int beam, int32_t *path_out, double *lpj_out);
/* my_suff_stat["lpj"] (N,S_perm+S) float64. */
int evoamd_upload_lpj(evoamd_ctx *ctx, const double *lpj);
int evoamd_download_lpj(evoamd_ctx *ctx, double *lpj);

/* ---- parameters Theta -------------------------------------------------------------- */
/* BSC: W (D,H) row-major, pi, sigma.  Performs E_step_precompute on the host side of the
 * library (bsc.py:99-125: pre1, pil_bar, ljc) and uploads W^T. ljc is returned. */
int evoamd_set_params_bsc(evoamd_ctx *ctx, const double *W, double pi, double sigma, double *ljc);
/* SSSC: W (D,H), pies (H), mus (H), Psi (H,H) row-major, sigma2.  pil_bar / ljc follow
 * sssc.py:328-366 (sigma2 through long double).  Launches the dense precompute
 * G = W^T W and B = Y W on the f64 matrix cores. */
int evoamd_set_params_sssc(evoamd_ctx *ctx, const double *W, const double *pies, const double *mus,
                           const double *Psi, double sigma2, double *ljc);

/* ---- E-step ------------------------------------------------------------------------ */
/* lpj of every resident state K^n under the current Theta -> device lpj[:, S_perm:]
 * (and the permanent all-zero column when S_perm = 1).  Includes the clamp of
 * Model.lpj_reset_check (_models.py:567-596).  Replaces the per-datapoint calls at
 * _models.py:508-512 / sssc.py:521-525 (BSC.log_pseudo_joint bsc.py:78-97,
 * SSSC.log_pseudo_joint sssc.py:241-326, *_permanent_states bsc.py:59-76, sssc.py:224-239). */
int evoamd_lpj_resident(evoamd_ctx *ctx);

/* Ragged candidate batch: cand_bool (N,Cmax,H) bool, counts (N,) int32 (counts[n] <= Cmax
 * rows of datapoint n are valid).  Evaluates lpj of every valid candidate against y_n and
 * keeps the batch + its lpj on the device for evoamd_vary_kn.  lpj_out (N,Cmax) may be
 * NULL.  Replaces the eval_lpj closure (_models.py:517-519, sssc.py:530-532). */
int evoamd_lpj_candidates(evoamd_ctx *ctx, const uint8_t *cand_bool, const int32_t *counts,
                          int Cmax, double *lpj_out);

/* Same batch layout, but with lpj values supplied by the caller (N,Cmax) instead of being
 * evaluated: installs the resident candidate batch for evoamd_vary_kn.  This is vary_Kn's own
 * calling shape (lpj_new, states_new given; variational/utils.py:231-244). */
int evoamd_set_candidates(evoamd_ctx *ctx, const uint8_t *cand_bool, const int32_t *counts,
                          int Cmax, const double *lpj);

/* One state set shared by ALL datapoints (the exact-likelihood path, _models.py:385-394):
 * states_bool (C,H); lpj_out (N,C) host. */
int evoamd_lpj_shared(evoamd_ctx *ctx, const uint8_t *states_bool, int C, double *lpj_out);

/* Single-datapoint operator with the reference's calling shape
 * (log_pseudo_joint(model_params, my_suff_stat, my_data): this_y (D,), this_states (C,H)
 * -> (C,)).  flags_out[3] receives {any NaN, any < finfo.min, any inf} for the caller's
 * reset counters. */
int evoamd_lpj_single(evoamd_ctx *ctx, const double *y, const uint8_t *states_bool, int C,
                      double *lpj_out, int32_t *flags_out);

/* K^n update on the device: de-duplicate the resident candidate batch against K^n (and
 * within itself, first occurrence wins), then swap the best accepted new states for the
 * worst evicted old ones exactly as vary_Kn does (variational/utils.py:231-337,
 * unification branch), writing K^n and lpj in place.  sums_out[2] += {#new unique,
 * #swapped} over this rank's datapoints (_models.py:537-538). */
int evoamd_vary_kn(evoamd_ctx *ctx, int Mprime, double *sums_out);

/* Device-side evolutionary candidate generation (fitness-proportional parents + random
 * bit flips, eas.py:10-43,138-146,153-313 for n_generations = 1), counter-based RNG: the
 * law of the reference, not np.random's draws; the stream is documented in
 * csrc/kernels_evolve.hpp and evo_amd.variational.evolve_randflip_counter repeats it bit for
 * bit.  Fills the resident candidate batch (slot p * n_children + i: child i of the p-th
 * drawn parent; vary_kn de-duplicates) and evaluates it. */
int evoamd_evolve_randflip(evoamd_ctx *ctx, int n_parents, int n_children, uint64_t seed,
                           int fit_parents);

/* Every operator of the reference's evolutionary algorithm on the device, any number of generations
 * (evolve_states eas.py:153-313): mutation 0 randflip (eas.py:10-43), 1 sparseflip (:46-100), 2 cross (:103-125),
 * 3 cross_randflip, 4 cross_sparseflip (:128-135); fit_parents 1 fitparents (:138-146) / 0 randparents (:149-150);
 * sparseness = model_params["piH"], bitflip_prob as in my_suff_stat (NaN when unused).  Per generation: parents from
 * K^n (generation 0) or from the previous generation's new states plus the known states its children duplicated --
 * with the lpj pairing of eas.py:284-293 as written (off by one when S_perm = 0) --, mutation, de-duplication against
 * [incl; K^n; earlier new states], lpj of the survivors.  The resident candidate batch then holds what
 * evolve_states returns (new_states[new_and_unique], lexicographic within a generation) for evoamd_vary_kn;
 * n_children_per_generation x n_generations <= Cmax.  Counter-based RNG as in evoamd_evolve_randflip, which stays
 * the fast path for randflip with one generation. */
int evoamd_evolve_states(evoamd_ctx *ctx, int mutation, int fit_parents, int n_parents, int n_children,
                         int n_generations, uint64_t seed, double sparseness, double bitflip_prob);
/* The resident candidate batch back to the host in the reference's layout: cand_bool (N,Cmax,H) bool bytes,
 * counts (N), lpj (N,Cmax) -- rows >= counts[n] are unspecified.  What evolve_states hands to vary_Kn
 * (eas.py:313), for callers that keep the reference's two-call structure, and for the distribution tests. */
int evoamd_download_candidates(evoamd_ctx *ctx, uint8_t *cand_bool, int32_t *counts, double *lpj);

/* K^n refined while Theta stays fixed: one pass over the resident K^n at entry, then n_iterations x (children, their
 * lpj, selection).  The selection kernel writes the lpj of every state it swaps in, so the rows stay current and no
 * iteration evaluates K^n again; no statistics pass runs and the fused E-step kernel is never used.  Iteration t draws
 * its children with seed0 + t * seed_stride (mod 2^64): evoamd_evolve_randflip's kernel for mutation 0 with one
 * generation and at most 8 children, evoamd_evolve_states' otherwise -- arguments and checks as for those two calls
 * and evoamd_vary_kn, results bit for bit those of the separate calls.  trace_out (n_iterations, 3): row t =
 * {Fs = sum_n logsumexp_s lpj_ns after iteration t, new unique states, swapped states} of this rank, per iteration
 * (not running sums).  patience <= 0: nothing waits for the device until the end.  patience > 0: after every
 * check_every iterations that chunk's rows are fetched and the loop ends there once the last `patience` rows all have
 * swapped / N <= min_sub; *n_done_out = iterations run (rows beyond are not written), and the result is what
 * n_iterations = *n_done_out without patience gives.  On return the lpj rows belong to the resident K^n, the
 * products of the last statistics pass are gone as after any selection, and the scalar block is as one evoamd_estep
 * with the last iteration's arguments leaves it: a following evoamd_stats reports that iteration's counts and Fs. */
int evoamd_refine_states(evoamd_ctx *ctx, int n_iterations, int mutation, int fit_parents, int n_parents,
                         int n_children, int n_generations, uint64_t seed0, uint64_t seed_stride, double sparseness,
                         double bitflip_prob, int Mprime, int check_every, int patience, double min_sub,
                         double *trace_out, int *n_done_out);

/* Local search on K^n at fixed Theta: a deterministic sweep of the one-flip neighbourhood of its best states
 * (csrc/kernels_sweep.hpp has the law; evo_amd.variational.sweep_states_host is the NumPy mirror).  Per datapoint the
 * n_parents varying states with the largest lpj (descending, ties by ascending slot) are the parents; every state that
 * differs from a parent in one latent is scored with the model's lpj in the Gram form of evoamd_seed_states, unless it is
 * the all-zero state, K^n holds it already (an exact test on the packed words) or it exceeds the seeding cap (ES3C 8,
 * EBSC 64 active latents); per parent the n_keep best scored neighbours (descending score, ties by ascending latent; a
 * score that is not finite is never proposed) go to the resident candidate batch, parent-major, then by rank.
 * evoamd_sweep_propose evaluates the resident rows (as evoamd_refine_states does at entry), runs the proposal kernel and
 * the model's own lpj kernels on the emitted rows -- clamp and reset counters as for E-step children -- and leaves the
 * batch for evoamd_vary_kn and evoamd_download_candidates; the sweep's scores only rank.  Outputs, each may be NULL:
 * score_out (N, Cmax) the score of every emitted row (NaN beyond counts[n]); from the best parent, best_flip_out (N) the
 * latent of its best scored neighbour or -1 and gain_out (N) that score minus the parent's own, -inf without a scored
 * neighbour (NaN: an ES3C parent above 8 latents has no score of its own) -- gain <= 0 certifies that the best state of
 * K^n has no better one-flip neighbour outside K^n; n_capped_out (N) the parents that lost a neighbour to the cap.
 * EVOAMD_E_INVALID before anything is written -- K^n, the rows and the candidate batch stay as they were -- without Theta,
 * data or K^n, with masks present (incomplete data needs the _ex calls below), with background_unit, ebsc_f32 or bsc_direct, for
 * n_parents outside [1, min(S, 64)], n_keep < 1, n_parents * n_keep > Cmax, and when the keys of one datapoint do not
 * fit a wavefront's share of LDS at this H.  No atomics, fixed summation order: two calls give the same bits. */
int evoamd_sweep_propose(evoamd_ctx *ctx, int n_parents, int n_keep, double *score_out, int32_t *best_flip_out,
                         double *gain_out, int32_t *n_capped_out);
/* n_sweeps x (the proposals above, selection with Mprime as evoamd_vary_kn): one pass over K^n at entry, after that the
 * selection kernel keeps the rows current, so on return they are bit for bit what evoamd_lpj_resident would give and the
 * result is that of the separate calls.  trace_out (n_sweeps, 3): row t = {Fs, new unique states, swapped states} of
 * sweep t, as for evoamd_refine_states, with the scalar block left as that call leaves it.  stop_when_quiet: the row is
 * fetched after each sweep and the loop ends after a sweep that swapped nothing; *n_done_out = sweeps run.  The
 * certificate outputs describe the last sweep run: after a quiet one, the final K^n.  Refusals as above, and for an
 * Mprime outside [1, S], n_sweeps < 1 or a NULL trace_out / n_done_out. */
int evoamd_sweep_states(evoamd_ctx *ctx, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                        double *trace_out, int *n_done_out, int32_t *best_flip_out, double *gain_out,
                        int32_t *n_capped_out);
/* The two calls above with flags (0: exactly those calls, every refusal and its text included).  EVOAMD_SWEEP_INCOMPLETE
 * permits incomplete data; it is a permission, not a mode, like EVOAMD_SEED_INCOMPLETE: with masks resident
 * (evoamd_upload_masks) the same law runs with the Gram quantities of the datapoint's reliable entries o = x_infr[n] --
 * G(n) = W_o^T W_o formed per datapoint from W and the resident mask, B_n = y_o^T W_o and |y_o|^2 as evoamd_upload_masks
 * left them (it zeroes the missing entries of Y, so NaN there is never read); Psi, mu, pil_bar, sigma2 and pre1 are not
 * masked -- the lpj that evoamd_lpj_resident and the candidate lpj kernels compute on masked data, which evaluate the
 * emitted rows.  A datapoint without a reliable entry is scored by the prior alone.  Without masks the complete kernel
 * runs, bit for bit as without the flag.  EBSC: the diagonal of G(n) once per datapoint and ONE sweep over W per parent
 * with the combined column r_d = sum_{i in p} W_di; ES3C: the rows of G(n) of a parent's first 9 active latents and the
 * diagonal, 10 rows of ceil64(H) doubles per wavefront, in LDS while they fit one wavefront's share, else in a buffer of
 * the context grown on demand.  Refusals as above, and for an unknown flag bit and for keys (8 H bytes, EBSC 24 H), a
 * staged column (8 D bytes) and a list of the reliable entries (4 D bytes) that do not fit one wavefront's share of LDS.
 * No atomics, a fixed summation order (ascending d, ascending i): two calls give the same bits. */
#define EVOAMD_SWEEP_INCOMPLETE 1u
int evoamd_sweep_propose_ex(evoamd_ctx *ctx, int n_parents, int n_keep, unsigned flags, double *score_out,
                            int32_t *best_flip_out, double *gain_out, int32_t *n_capped_out);
int evoamd_sweep_states_ex(evoamd_ctx *ctx, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                           unsigned flags, double *trace_out, int *n_done_out, int32_t *best_flip_out, double *gain_out,
                           int32_t *n_capped_out);
/* The swap neighbourhood beside the one-flip one (csrc/kernels_sweep_swap.hpp has the law;
 * evo_amd.variational.swap_states_host is the NumPy mirror): one active latent a of a parent switched off and one inactive
 * latent j switched on, every pair (a, j) scored with the model's lpj unless K^n holds that state (an exact test on the
 * packed words) or the parent exceeds the seeding cap (ES3C 8, EBSC 64 active latents: none of its swaps is scored); per
 * parent the n_keep best (descending score, ties by ascending a, then ascending j) are appended behind the rows of the
 * flip stage, parent-major, then by rank.  Flags: EVOAMD_SWEEP_SWAP scores swaps too, EVOAMD_SWEEP_NO_FLIP (valid only
 * together with it) leaves the flip stage out; with neither bit the _nb calls are exactly the _ex calls.  With both
 * stages on each gets up to n_keep rows per parent and 2 * n_parents * n_keep <= Cmax is required, with one stage
 * n_parents * n_keep <= Cmax.  Outputs, each (and out itself) may be NULL: score, best_flip, gain, n_capped as above
 * (the three of the flip stage are not written with EVOAMD_SWEEP_NO_FLIP); from the best parent best_swap (N, 2) = (a, j) of
 * its best scored swap or (-1, -1) and swap_gain (N) that score minus the parent's own, -inf without a scored swap;
 * n_capped_swap (N) the parents above the cap.  After a quiet sweep with both stages on, gain <= 0 and swap_gain <= 0
 * certify that the best state of K^n has no better one-flip or swap neighbour outside K^n.  In the loop call "quiet" means
 * that the sweep swapped nothing into K^n.  Refusals, before anything is written: everything the calls above refuse,
 * EVOAMD_SWEEP_SWAP together with EVOAMD_SWEEP_INCOMPLETE or with masks resident (swaps on incomplete data are not
 * supported), EVOAMD_SWEEP_NO_FLIP without EVOAMD_SWEEP_SWAP, the quota rule, and an LDS share that does not fit.  No atomics,
 * fixed summation order: two calls give the same bits. */
#define EVOAMD_SWEEP_SWAP 2u
#define EVOAMD_SWEEP_NO_FLIP 4u
typedef struct evoamd_sweep_out {
  double *score;          /* (N, Cmax) */
  int32_t *best_flip;     /* (N) */
  double *gain;           /* (N) */
  int32_t *n_capped;      /* (N) */
  int32_t *best_swap;     /* (N, 2) */
  double *swap_gain;      /* (N) */
  int32_t *n_capped_swap; /* (N) */
} evoamd_sweep_out;
int evoamd_sweep_propose_nb(evoamd_ctx *ctx, int n_parents, int n_keep, unsigned flags, const evoamd_sweep_out *out);
int evoamd_sweep_states_nb(evoamd_ctx *ctx, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                           unsigned flags, double *trace_out, int *n_done_out, const evoamd_sweep_out *out);

/* The neighbourhood bound: the exact mass of the one-flip neighbours of the best states of K^n (csrc/kernels_nbound.hpp has
 * the law; evo_amd.variational.neighbour_bound_host is the NumPy mirror).  Per datapoint the n_parents varying states with
 * the largest lpj are the parents, as for evoamd_sweep_propose but up to S of them; every state one flip away from a parent
 * is scored with the sweep's own scores unless it is the all-zero state, K^n holds it, it exceeds the seeding cap (ES3C 8,
 * EBSC 64 active latents) or an earlier parent owns it -- exact tests on the packed words, so every state of the union of
 * the neighbourhoods outside K^n is counted exactly once -- and the scores are summed, not ranked:
 * M_n = log sum exp(score), F+_n = logaddexp(F_n, M_n) with F_n evoamd_posterior_scores' bound, F_n <= F+_n <= log p(y_n) - ljc.
 * A deterministic lower bound: no random numbers, no atomics on global memory, a fixed summation order, two calls give the
 * same bits.  The call evaluates the resident rows (as evoamd_sweep_propose does at entry) and writes nothing into K^n, the
 * candidate batch or the statistics rows.  Outputs (host, N each, each pointer and out itself may be NULL): F; M (-inf
 * without a scored neighbour); n_states, the neighbours summed; n_capped, the parents that lost a neighbour to the cap;
 * best_score, best_parent (the parent's rank) and best_flip (the latent) of the largest score, ties by ascending rank, then
 * latent (-inf / -1 / -1 without one); sum (2) = {the sum of F+_n over the datapoints with an estimate, their number}.  A
 * row with a NaN or +inf, or all -inf ("bad weights", as evoamd_loglik_estimate): F and M NaN, the counts 0, no estimate.
 * flags: EVOAMD_NBOUND_INCOMPLETE permits incomplete data, a permission like EVOAMD_SWEEP_INCOMPLETE: with masks resident the
 * masked instantiation runs, without masks the complete one.  EVOAMD_E_INVALID before anything is written: an unknown flag;
 * no Theta, data or K^n; masks resident without the flag; background_unit, ebsc_f32 or bsc_direct; n_parents outside [1, S];
 * one wavefront's share of LDS (the flip sweep's with n_keep = 0 plus 8 S bytes) too large. */
#define EVOAMD_NBOUND_INCOMPLETE 1u
typedef struct evoamd_nbound_out {
  double *F;            /* (N) */
  double *M;            /* (N) */
  int32_t *n_states;    /* (N) */
  int32_t *n_capped;    /* (N) */
  double *best_score;   /* (N) */
  int32_t *best_parent; /* (N) */
  int32_t *best_flip;   /* (N) */
  double *sum;          /* (2) */
} evoamd_nbound_out;
int evoamd_neighbour_bound(evoamd_ctx *ctx, int n_parents, unsigned flags, const evoamd_nbound_out *out);

/* Annealed importance sampling: stochastic lower and upper bounds on log p(y_n) - ljc that do not depend on K^n
 * (csrc/kernels_ais.hpp has the law; evo_amd.models.ais_log_likelihood_counter is the NumPy mirror).  EBSC; incomplete data under EVOAMD_AIS_INCOMPLETE.
 * Per datapoint n_chains Gibbs chains of n_temps temperatures, one wavefront per (datapoint, chain); betas: the float64
 * schedule of n_temps + 1 values, 0 = betas[0] < betas[1] <= ... <= betas[n_temps] = 1 (host); seed / first_index: the
 * counter stream of evoamd_generate (datapoint n is index first_index + n of the data set; chain c draws under purpose
 * AIS_PURPOSE + c, one uniform per (c, t, h): chain c does not depend on n_chains, shards concatenate).
 * flags: 0 = forward chains from the prior (ll: a lower bound in expectation); EVOAMD_AIS_REVERSE = chains from s_start
 * back to the prior (ll: an upper bound in expectation, PROVIDED row n of s_start is an exact posterior sample, which it is
 * only when y_n was generated from this Theta with that s); s_start: (N, ceil(H / 64)) words in the layout of K^n (host).
 * EVOAMD_AIS_ADMIT (forward only): the final states of the first min(n_chains, Cmax) chains become the candidate batch in
 * chain order, the all-zero state skipped, digests written where in use; the model's candidate lpj kernels evaluate them
 * and the selection (vary_kn with Mprime) runs -- the tail of a sweep; the resident rows are evaluated first, as a sweep
 * does at entry.  Without it K^n, lpj, the candidate batch and the statistics rows are not written (Mprime is not read).
 * Outputs (host; each pointer and out itself may be NULL): ll, ess, log_w_mean, log_w_min, log_w_max (N doubles), n_flips
 * (N int64, the accepted flips of all chains), log_w (N, n_chains), final_words (N, n_chains, ceil(H / 64)) in the layout
 * of K^n, chain_flips (N, n_chains: the accepted flips of each chain), sum (1) = the sum of ll in datapoint order; with EVOAMD_AIS_ADMIT F_before / F_after (N, the bound of K^n without
 * ljc around the selection) and admit_sums (2) = {sum of the new unique states, sum of the substitutions}, as evoamd_vary_kn.
 * Deterministic: two calls give the same bits.  EVOAMD_E_INVALID before anything is written, each with its own text: an
 * unknown flag; no Theta or data; ES3C; the float32 mode (ebsc_f32); background_unit; bsc_direct; masks resident; H > 1024;
 * n_chains < 1; n_temps < 1; betas NULL, not starting at 0, not ending at 1, or descending; EVOAMD_AIS_REVERSE without
 * s_start; EVOAMD_AIS_ADMIT with EVOAMD_AIS_REVERSE, without K^n or with Mprime outside [1, S].
 * EVOAMD_AIS_INCOMPLETE: a permission, like EVOAMD_SEED_INCOMPLETE -- with masks resident (evoamd_upload_masks) the chains run
 * on the datapoint's own G(n) = W_o^T W_o over its reliable entries o, a row formed from W and the mask when a flip happens
 * (products rounded and added in ascending d; kernels_ais.hpp, INCOMPLETE DATA); B and yy are the resident, masked ones, so
 * values of y under False never enter.  A datapoint without a reliable entry is not skipped: prior draws, log w = 0.  With
 * EVOAMD_AIS_ADMIT the candidate lpj kernels and the selection run masked as in every E-step.  Without masks the flag
 * changes nothing; masks without the flag are refused as before.  Refused with the flag: a D whose column and list (D
 * doubles + D ints per wavefront) do not fit into the 160 KiB of a compute unit beside the rows over H. */
#define EVOAMD_AIS_REVERSE 1u
#define EVOAMD_AIS_ADMIT 2u
#define EVOAMD_AIS_INCOMPLETE 8u /* (4u stays unassigned: callers have been promised "unknown flag" for it) */
typedef struct evoamd_ais_out {
  double *ll;            /* (N) */
  double *ess;           /* (N) */
  double *log_w_mean;    /* (N) */
  double *log_w_min;     /* (N) */
  double *log_w_max;     /* (N) */
  int64_t *n_flips;      /* (N) */
  double *log_w;         /* (N, n_chains) */
  uint64_t *final_words; /* (N, n_chains, ceil(H / 64)) */
  int32_t *chain_flips;  /* (N, n_chains) */
  double *F_before;      /* (N), EVOAMD_AIS_ADMIT */
  double *F_after;       /* (N), EVOAMD_AIS_ADMIT */
  double *admit_sums;    /* (2), EVOAMD_AIS_ADMIT */
  double *sum;           /* (1) */
} evoamd_ais_out;
int evoamd_ais_loglik(evoamd_ctx *ctx, int n_chains, int n_temps, const double *betas, uint64_t seed, uint64_t first_index,
                      unsigned flags, const uint64_t *s_start, int Mprime, const evoamd_ais_out *out);

/* Posterior expectations beyond K^n: weighted marginals E_p[s_h | y_n] and means from the forward chains of
 * evoamd_ais_loglik, continued (csrc/kernels_ais_post.hpp has the law; evo_amd.models.ais_posterior_counter is the NumPy
 * mirror).  evoamd_posterior_codes, evoamd_reconstruct and evoamd_predictive_moments are expectations under q_n, the posterior
 * truncated to K^n, and evoamd_loglik_exact with marginals stops at H of about 30; this call goes beyond both: a forward chain
 * with its weight is a properly weighted sample of the TRUE posterior.  EBSC, H <= 1024; incomplete data: evoamd_ais_posterior_ex.
 * The chains are those of evoamd_ais_loglik with flags = 0 (same stream, start and schedule): the scan at betas[n_temps] = 1
 * is the first of n_keep >= 1 KEPT scans, the others follow at beta = 1 with the uniform blocks n_temps + 2, ...; in a kept
 * scan the conditional p(s_h = 1 | the rest) is added to R_c[h] when latent h is decided (Rao-Blackwell), r_ch = R_c[h] /
 * n_keep; after each kept scan the chain compares lpj of its state with the best it has seen.  Per datapoint, with a_c the
 * normalised weights: p = sum_c a_c r_c., p_se = sqrt(sum_c (a_c (r_c. - p))^2), count = sum_h p_h, map_lpj / map_state =
 * the best state over the chains (ties: the lowest chain), ll / ess / log_w_* / n_flips as evoamd_ais_loglik (n_flips counts
 * the kept scans too).  mean (N, D) = p W^T, the posterior mean of W s, through the f64 GEMM into a buffer of its own.
 * block_datapoints: 0 = the datapoints are walked in blocks whose per-chain rows (block x n_chains x 64 ceil(H / 64) doubles)
 * stay within 256 MiB; > 0 = that many per block (for tests; the same limit holds).  Results do not depend on it.
 * Outputs (host; each pointer and out itself may be NULL): p, p_se (N, H), count, map_lpj, ll, ess, log_w_mean, log_w_min,
 * log_w_max (N), n_flips (N int64), map_state (N, ceil(H / 64)) words in the layout of K^n, mean (N, D), and per chain log_w,
 * chain_map_lpj (N, n_chains), rb (N, n_chains, H), chain_map_state (N, n_chains, ceil(H / 64)), chain_flips (N, n_chains).
 * Nothing of the EM state is written: not K^n, lpj, the candidate batch or the statistics rows, not y_hat or its validity
 * (B = Y W is (re)formed like by every lpj pass).  Deterministic: two calls give the same bits.  No reverse chains, no admit.
 * EVOAMD_E_INVALID before anything is written, each with its own text: no Theta or data; ES3C; the float32 mode (ebsc_f32);
 * background_unit; bsc_direct; masks resident; H > 1024; n_chains < 1; n_temps < 1; n_keep < 1; betas NULL, not starting at
 * 0, not ending at 1, or descending; block_datapoints < 0 or one block's rows above 256 MiB. */
typedef struct evoamd_ais_post_out {
  double *p;                 /* (N, H) */
  double *p_se;              /* (N, H) */
  double *count;             /* (N) */
  double *map_lpj;           /* (N) */
  uint64_t *map_state;       /* (N, ceil(H / 64)) */
  double *ll;                /* (N) */
  double *ess;               /* (N) */
  double *log_w_mean;        /* (N) */
  double *log_w_min;         /* (N) */
  double *log_w_max;         /* (N) */
  int64_t *n_flips;          /* (N) */
  double *mean;              /* (N, D) */
  double *log_w;             /* (N, n_chains) */
  double *rb;                /* (N, n_chains, H) */
  double *chain_map_lpj;     /* (N, n_chains) */
  uint64_t *chain_map_state; /* (N, n_chains, ceil(H / 64)) */
  int32_t *chain_flips;      /* (N, n_chains) */
} evoamd_ais_post_out;
int evoamd_ais_posterior(evoamd_ctx *ctx, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                         uint64_t first_index, int64_t block_datapoints, const evoamd_ais_post_out *out);
/* evoamd_ais_posterior with flags: 0 = that call; EVOAMD_AIS_INCOMPLETE admits resident masks as for evoamd_ais_loglik (the
 * chains on G(n) of the reliable entries; mean = p W^T covers every entry, the missing ones included).  Any other flag, and
 * a D that does not fit into LDS, is EVOAMD_E_INVALID before anything is written. */
int evoamd_ais_posterior_ex(evoamd_ctx *ctx, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                            uint64_t first_index, int64_t block_datapoints, unsigned flags, const evoamd_ais_post_out *out);

/* "Rescue": evoamd_ais_posterior_ex on LISTED datapoints, and the best distinct states its chains visited handed to K^n.
 * index (n_index int64, strictly ascending, each in [0, N)): the chains run for these datapoints only, and every output
 * of evoamd_ais_post_out has n_index rows in list order -- row i is bit for bit row index[i] of the call without a list
 * at the same seed (the stream of row i is that of data set index first_index + index[i]; blocks run over list
 * positions).  index NULL (n_index 0): all N datapoints.  n_index = 0 with a list: nothing runs, nothing is written.
 * flags: EVOAMD_AIS_INCOMPLETE as for _ex; EVOAMD_AIS_ADMIT: after the chains and the fold (csrc/kernels_ais_post.hpp,
 * ADMISSION, has the law; evo_amd.models.ais_admit_candidates_host is the NumPy mirror of the emission) the resident
 * rows are evaluated, then per listed datapoint the chains' best states -- ranked by their lpj descending, ties to the
 * lower chain, chains with a lpj that is not finite left out; the all-zero state, repeats of a state ranked before and
 * states K^n holds dropped; at most Cmax -- become its rows of the candidate batch (count 0 for every other datapoint),
 * the candidate lpj kernels and the selection with Mprime run as in every E-step (masked with masks resident), and
 * the outputs below are written, n rows each (n = n_index, or N): F_before / F_after (the bound of K^n without ljc),
 * n_distinct (distinct non-zero best states), n_new (those K^n did not hold), n_proposed = min(n_new, Cmax),
 * n_admitted (the proposed states K^n holds after the selection), map_held_before / map_held_after (0 / 1: K^n holds
 * map_state), admit_sums (2: the selection's sums as evoamd_vary_kn).  Without EVOAMD_AIS_ADMIT nothing of the EM state
 * is written and the added outputs are not touched.
 * EVOAMD_E_INVALID before anything is written, each with its own text: everything evoamd_ais_posterior_ex refuses; any
 * other flag; n_index < 0; an index outside [0, N), repeated or descending (the first offender is named); with
 * EVOAMD_AIS_ADMIT K^n not on the device and Mprime outside [1, S]. */
typedef struct evoamd_ais_post_sel_out {
  evoamd_ais_post_out post;  /* rows: the listed datapoints */
  double *F_before;          /* (n), EVOAMD_AIS_ADMIT, like the rest */
  double *F_after;           /* (n) */
  int32_t *n_distinct;       /* (n) */
  int32_t *n_new;            /* (n) */
  int32_t *n_proposed;       /* (n) */
  int32_t *n_admitted;       /* (n) */
  int32_t *map_held_before;  /* (n) */
  int32_t *map_held_after;   /* (n) */
  double *admit_sums;        /* (2) */
} evoamd_ais_post_sel_out;
int evoamd_ais_posterior_sel(evoamd_ctx *ctx, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                             uint64_t first_index, int64_t block_datapoints, unsigned flags, const int64_t *index,
                             int64_t n_index, int Mprime, const evoamd_ais_post_sel_out *out);
/* TEST-ONLY: the emission kernel of EVOAMD_AIS_ADMIT alone, on the caller's best_lpj (n, n_chains) and best (n, n_chains,
 * ceil(H / 64) words in the layout of K^n) for the rows index (n = n_index; NULL: the N datapoints), against the
 * resident K^n.  It leaves the candidate batch installed and evaluated (evoamd_download_candidates reads it) and
 * returns n_distinct, n_new, n_proposed, map_held (n each), the candidates' digests (dig_out (N, Cmax), rows below a
 * datapoint's count) where digests are in use, and whether they are (*dig_used). */
int evoamd_ais_post_admit_probe(evoamd_ctx *ctx, const double *best_lpj, const uint64_t *best, int n_chains,
                                const int64_t *index, int64_t n_index, int32_t *n_distinct, int32_t *n_new,
                                int32_t *n_proposed, int32_t *map_held, uint64_t *dig_out, int *dig_used);

/* Per-datapoint scores of the lpj rows and K^n resident on the device (after a seed, an upload or any pass), each output
 * (N) or NULL.  With m = max_s lpj_ns, w_s = exp(lpj_ns - m), z = sum_s w_s over the S_perm + S columns:
 * F_out = m + log z (the bound per datapoint without ljc, the counterpart of ll_out of evoamd_loglik_exact);
 * entropy_out = log z - sum_s w_s (lpj_ns - m) / z, the entropy of q_n (weights that underflow to 0 contribute 0);
 * best_out = the first column of the row that holds m; k_best_out = active latents of that state (0 for the permanent
 * all-zero column); k_mean_out = sum_s q_ns |s_s|.  Counts come from the packed words.  Fixed reduction order: two
 * calls give the same bits.  Nothing of the EM state changes. */
int evoamd_posterior_scores(evoamd_ctx *ctx, double *F_out, double *entropy_out, int32_t *best_out,
                            int32_t *k_best_out, double *k_mean_out);

/* ---- M-step sufficient statistics + free energy ------------------------------------- */
/* Number of doubles in the packed accumulator for the configured model:
 *   BSC : Wp (H,D) | Wq (H,H) | pies (H) | sigma | tail[8]
 *   SSSC: xpt_s (H) | xpt_ss (H,H) | xpt_sz (H) | xpt_szsz (H,H) | Wp (D,H) | s_sz_outer (H,H) |
 *         sz_sz_outer (H,H) | y_outer_diag (D) | tail[8]
 *   tail = { Fs, sum_nunique, sum_sub, N, reset_isnan, reset_smaller_eps, reset_isinf, 0 } */
int64_t evoamd_acc_size(evoamd_ctx *ctx);
/* Computes the per-rank sums from the resident K^n / lpj (bsc.py:176-223;
 * sssc.py:553-646,761; free energy _models.py:544-546), all-reduces them over the RCCL
 * communicator if one is attached (bsc.py:230-231,257,274; sssc.py:671-691,763,773-780),
 * and copies the packed result to acc_out (host). */
int evoamd_stats(evoamd_ctx *ctx, double *acc_out);
/* Device-resident M-step: computes the statistics like evoamd_stats (incl. the
 * all-reduce) but leaves them on the device, then evaluates the Theta update (bsc.py:226-277 /
 * sssc.py:687-770), the clamps of check_params (_models.py:101-159) and E_step_precompute on the
 * GPU and installs the result as the context's current parameters.  learn_mask bits: 1 W, 2 pies
 * (BSC: pi), 4 mus, 8 sigma2 (BSC: sigma), 16 Psi; 0 = statistics only; 32 = also form the data estimate under the OLD
 * Theta (evoamd_reconstruct); 64 = Theta^new stays on the device (otherwise it rides along into pinned host memory,
 * where evoamd_get_params_* finds it: what step() of the reference hands back) -- the caller fetches it with
 * evoamd_get_params_* when it looks at it (evo_amd.models: lazy_theta=True).  tail_out[8] = accumulator
 * tail, dpar_out[16] = scalar block of the NEW Theta (kernels_mstep.hpp: DP_*; [8] = ljc of the Theta
 * the E-step used when learn_mask != 0, else [3] is).  The H x H systems (Gram-type moment matrices) are inverted by
 * block Gauss-Jordan with the 16 / 32-column diagonal blocks as pivots (options "inverse_spd", "inverse_block"); a
 * pivot block that is not safely positive repeats the update with the partially pivoted elimination.  An exactly
 * singular system -- or one so ill-conditioned that Theta^new is not finite -- returns EVOAMD_E_SINGULAR with
 * tail_out / dpar_out filled in (dpar_out[7] = 1 singular, 2 non-finite): the E-step results stand, Theta on the device is
 * invalid, and the caller finishes the step with the reference's lstsq / pinv fallbacks (bsc.py:236-250,
 * sssc.py:692-708; evo_amd.models does) and installs a Theta with evoamd_set_params_*. */
int evoamd_mstep_device(evoamd_ctx *ctx, int learn_mask, double *tail_out, double *dpar_out);
/* Incomplete data (examples/image-inpainting/main.py:105-111); EBSC as described, ES3C:
 * every state goes through the wavefront kernel, which forms G_A = W_obs^T W_obs of its datapoint
 * (sssc.py:276-318), the statistics pass always forms y_hat (it needs reconstruct_in_stats, sssc.py:630-633)
 * and leaves sum over reliable entries of y_hat^2 in the accumulator tail[7] (sssc.py:640-645,751).  x_infr (N x D bool
 * bytes): reliable entries -- only they enter lpj (bsc.py:59-97), the allzero term and the sigma sum
 * (bsc.py:206-219); x (N x D, NULL = x_infr): entries that keep their value in y_reconstructed.  Call after
 * evoamd_upload_data (missing entries of Y may hold NaN; the device copy zeroes them).  All lpj entry
 * points then use the direct residual kernel with the mask (a Gram form would need W_obs^T W_obs per
 * datapoint).  The M-step's Wp contraction reads y_reconstructed (bsc.py:184-189): either
 * evoamd_set_option(ctx, "reconstruct_in_stats", 1) before evoamd_stats (it then forms
 * y_hat = Es W^T and y_rec = x ? y : y_hat first; fetch y_hat with evoamd_reconstruct), or hand over an
 * older one with evoamd_upload_yrec.  The rows the Wp contraction reads skip a datapoint without a reliable entry for
 * EBSC (_models.py:648-649) and reconstruct it for ES3C, whose own loop has no such test (sssc.py:613-627,632).  EBSC's
 * sigma sum reads y_reconstructed at the reliable entries too (bsc.py:187,214-216): where x drops a reliable entry the
 * estimate enters, not the datum -- a correction launched only when x differs from x_infr; with x == x_infr an uploaded
 * y_reconstructed is taken to hold y at the reliable entries.  x_infr == NULL returns to complete data (upload Y again);
 * evoamd_configure drops the masks too.  evoamd_mstep_device handles incomplete data once evoamd_set_reliable_fraction
 * was called. */
int evoamd_upload_masks(evoamd_ctx *ctx, const uint8_t *x_infr, const uint8_t *x);
int evoamd_upload_yrec(evoamd_ctx *ctx, const double *y_reconstructed);
/* Incomplete data with the device Theta update (evoamd_mstep_device): the mean number of reliable
 * entries per datapoint over ALL ranks, sum(x_infr) / N.  bsc.py:113-118 / sssc.py:352-357 put it into
 * the Gaussian normaliser of ljc, bsc.py:266-272 / sssc.py:747-755 into the sigma / sigma2 update (as
 * written there: the old variance times the count of reliable entries is added to the residual sum).
 * Negative: complete data (default).  Call before evoamd_set_params_bsc / _sssc. */
int evoamd_set_reliable_fraction(evoamd_ctx *ctx, double reliable_per_datapoint);
/* evoamd_lpj_single with this datapoint's x_infr row (D bool bytes): log_pseudo_joint reading
 * my_data["this_x_infr"] (bsc.py:80-95).  Needs no resident masks (ES3C: it then forms the W^T of the current Theta
 * itself). */
int evoamd_lpj_single_masked(evoamd_ctx *ctx, const double *y, const uint8_t *x_infr, const uint8_t *states, int C,
                             double *lpj_out, int32_t *flags_out);
/* Posterior-predictive data estimate (complete data): y_hat (N x D, host) with
 *   y_hat[n] = sum_s q_ns W s / sum_s q_ns = W . E_q[s]           EBSC  (_models.py:614-665, bsc.py:279-287)
 *   y_hat[n] = sum_s q_ns W (s o kappa_ns) / sum_s q_ns = W . E_q[s o z]   ES3C  (sssc.py:368-405,613-627)
 * under the Theta and K^n of the last statistics pass -- what Model.reconstruct / EM_step(do_reconstruction)
 * write into my_data["y_reconstructed"] where my_data["x"] is False (the host applies that mask).
 * Call after evoamd_stats and before new parameters are set, or pass learn_mask | 32 to
 * evoamd_mstep_device, which then forms y_hat before it updates Theta. */
int evoamd_reconstruct(evoamd_ctx *ctx, double *y_hat);
/* The M-step's H x H solver on its own: A (and B if not NULL) are replaced by their inverses
 * (row-major n x n, n == H of the configured context).  This is the Gauss-Jordan code path that
 * evoamd_mstep_device uses in place of np.linalg.inv (sssc.py:693,738) / lstsq (bsc.py:237);
 * exported so that the parity tests can drive it with pivoting and near-singular cases.
 * timing_ms (may be NULL) receives the device time of the inversion. */
int evoamd_inverse(evoamd_ctx *ctx, double *A, double *B, int n, double *timing_ms);
/* The M-step's dense contraction on its own: C (M x Nc, row-major) = A^T B with A (K x M) and B (K x Nc)
 * row-major host arrays -- the f64 MFMA path behind Wp = Es^T Y (bsc.py:211 summed over n) and
 * [Y | Es | Ez]^T Ez (sssc.py:634,637,646), with the same tile-size / K-split / XCD dispatch as the
 * statistics pass.  sym_row0 >= 0 declares rows sym_row0.. of C symmetric (X^T X).  Exported for the
 * parity tests (the long-K tile variants only run at sizes no oracle fixture reaches). */
int evoamd_gemm_tn(evoamd_ctx *ctx, const double *A, const double *B, double *C, int64_t K, int M, int Nc,
                   int sym_row0);
/* TEST-ONLY: one dense kernel launch through the launcher the hot path calls, with the strides, base alignments and
 * options the real callers use (tests/test_gpu_dense.py; DESIGN "Dense probe").  Every operand is a whole padded host
 * buffer: `off` elements, then `guard` rows, the logical rows, `guard` rows, each row `ld` elements long; the probe
 * uploads all of it, passes base = buffer + off + guard * ld, and downloads all of C (and of `side`), so the caller
 * sees every element the kernel could have touched near its operands.
 *   op TN        C (M x Nc) = A^T B, A (K x M), B (K x Nc) double           -- launch_gemm_tn, every GemmTnOpts field;
 *                same_operand: B is A (the Gram route); diag != 0: `side` is diag(C), guard + M + guard doubles
 *      TN_F32    the same with float A, B and double C                      -- launch_gemm_tn_f32 (reads spare)
 *      NN        C (M x Nc) = A B, A (M x K)                                -- launch_gemm_nn_raw; ldct > 0: `side` is
 *                C^T, (guard + Nc + guard) x ldct (written by the parameter-sized kernel only)
 *      ROWS      C (M x Nc) = A^T B, whole K per 128-tile, plain stores     -- the B = Y W launch from Y^T
 *      ROWS_F32  the same in float; A2 (M x K, lda2) is the row-major copy the one-thread-per-element form reads
 *      COLSUM / COLSUM_SQ  C (1 x M) += column sums (of squares) of A (K x M) -- launch_colsum
 * route (may be NULL) receives what the launcher recorded: which kernel, tile, K splits, grouped chunks J, workgroups
 * per XCD, workspace slabs per workgroup, whether the workspace was used, and the device's compute units. */
#define EVOAMD_DENSE_TN 0
#define EVOAMD_DENSE_TN_F32 1
#define EVOAMD_DENSE_NN 2
#define EVOAMD_DENSE_ROWS 3
#define EVOAMD_DENSE_ROWS_F32 4
#define EVOAMD_DENSE_COLSUM 5
#define EVOAMD_DENSE_COLSUM_SQ 6
#define EVOAMD_ROUTE_NONE 0
#define EVOAMD_ROUTE_GRAM_SMALL 1
#define EVOAMD_ROUTE_TN64_SCALAR 2
#define EVOAMD_ROUTE_TN64_VEC 3
#define EVOAMD_ROUTE_TN128_SPLIT 4
#define EVOAMD_ROUTE_TN128_STREAMK 5
#define EVOAMD_ROUTE_TN128_GROUPED 6
#define EVOAMD_ROUTE_F32_STREAMK 7
#define EVOAMD_ROUTE_F32_GROUPED 8
#define EVOAMD_ROUTE_F32_NAIVE 9
#define EVOAMD_ROUTE_NN_SMALL 10
#define EVOAMD_ROUTE_NN_VEC 11
#define EVOAMD_ROUTE_NN_SCALAR 12
#define EVOAMD_ROUTE_ROWS 13
#define EVOAMD_ROUTE_ROWS_F32_STORE 14
#define EVOAMD_ROUTE_ROWS_F32_NAIVE 15
#define EVOAMD_ROUTE_COLSUM 16
typedef struct evoamd_dense_desc {
  int32_t op;
  int32_t M, Nc;
  int64_t K;
  int32_t lda, ldb, ldc, lda2, ldct;
  int32_t off_a, off_b, off_c; /* elements in front of each padded buffer: an odd one takes the base off 16 bytes */
  int32_t same_operand;
  int32_t deterministic, sym_row0, c_is_zero, accumulate, mirror, spare, diag;
  int32_t guard;
} evoamd_dense_desc;
typedef struct evoamd_dense_route {
  int32_t route, tile, splits, J, wpx, segmax, ws, n_cu;
} evoamd_dense_route;
int evoamd_dense_probe(evoamd_ctx *ctx, const evoamd_dense_desc *d, const void *A, const void *B, const void *A2,
                       void *C, void *side, evoamd_dense_route *route);
/* Current parameters of the context back to the host (after evoamd_mstep_device). */
int evoamd_get_params_bsc(evoamd_ctx *ctx, double *W, double *pi, double *sigma);
int evoamd_get_params_sssc(evoamd_ctx *ctx, double *W, double *pies, double *mus, double *Psi,
                           double *sigma2);
/* evoamd_mstep_device with bit 64 (Theta^new stays on the device) keeps the parameters the E-step ran with in a device
 * backup while the update overwrites them in place.  This call re-installs that backup -- what the caller needs when the
 * update returns EVOAMD_E_SINGULAR and it wants to finish the step with the reference's host formulas and fallbacks
 * (sssc.py:692-708, bsc.py:236-250), which start from the OLD Theta.  evoamd_get_params_* then reads them; the derived
 * tables are rebuilt by the next evoamd_set_params_*. */
int evoamd_restore_theta_backup(evoamd_ctx *ctx);
/* The whole E-step of the device-RNG path in one call -- the body of the reference's per-datapoint loop
 * (evo/models/_models.py:497-538, evo/models/sssc.py:510-552) for every datapoint of the shard: lpj of the resident K^n
 * (log_pseudo_joint), evolve_states with fitparents / randparents + randflip x 1 generation (evo/variational/eas.py:153-313),
 * lpj of the children, vary_Kn (evo/variational/utils.py:231-337); K^n, lpj rows and the row statistics of the M-step are
 * updated in place, the free-energy term and the counters go to the scalar block.  Equivalent to evoamd_lpj_resident +
 * evoamd_evolve_randflip + evoamd_vary_kn with the same arguments, bit for bit; where the shape allows it (ES3C, complete
 * data, digests, S_perm = 0, <= 64 children, H <= 1024) and option "fused_estep" asks for it, ONE kernel does it with a wave
 * per datapoint (the resident states above two latents by the list kernels in front of it).
 * *fused_out (may be NULL): 1 if the fused kernel ran. */
int evoamd_estep(evoamd_ctx *ctx, int n_parents, int n_children, uint64_t seed, int fit_parents, int Mprime, int *fused_out);
/* Diagnostics of evoamd_estep: out = { calls that ran the fused kernel, calls that ran the separate passes, datapoints the
 * last fused call's first launch left to the second (a child above 16 active latents), 0 }.  Synchronises the stream. */
int evoamd_estep_counters(evoamd_ctx *ctx, int64_t out[4]);
/* Fs only (sum_n logsumexp) of an arbitrary host lpj matrix (N,C) -- exact-likelihood path. */
int evoamd_free_energy(evoamd_ctx *ctx, const double *lpj, int64_t N, int C, double *Fs_out);
/* Exact log-likelihood terms over ALL states of the Hv = H - background latents that vary (1 <= Hv <= 32), without a
 * state table and without an N x 2^Hv array: the states are produced on the device in chunks of `chunk_states` (a power
 * of two >= 64; 0 = automatic: N x chunk doubles <= 512 MB, chunk <= 65536), each chunk is evaluated like an
 * evoamd_lpj_shared batch (same preconditions: configure, upload_data, set_params_*; incomplete data included) and
 * folded into a running log-sum-exp per datapoint.  background = 0: all 2^Hv states, the all-zero state's term as the
 * permanent state's (the reference's forced S_perm = 1, _models.py:366-373); background = 1: every state of the first
 * H - 1 latents with latent H - 1 on, no all-zero term (_models.py:389-390).  State index g has latent h on iff bit h of g.
 * ll_out (N, may be NULL): ll_n = logsumexp_s lpj_ns;  marg_out (N x H, may be NULL): the exact posterior marginals
 * E_p[s_h | y_n] (the background unit's column is 1);  *Fs_out = sum_n ll_n, summed in a fixed order.  Two calls with
 * the same inputs and chunk size give the same bits.  K^n, lpj, candidates, statistics rows, a prefetched pass and the
 * resident reconstruction stay as they are.  EVOAMD_E_SINGULAR / EVOAMD_E_KLIMIT as for evoamd_lpj_shared. */
int evoamd_loglik_exact(evoamd_ctx *ctx, int background, int chunk_states, double *ll_out, double *marg_out,
                        double *Fs_out);
/* Adds the E-step scalars produced outside evoamd_stats (e.g. host-side vary_Kn counts)
 * into the accumulator tail before the all-reduce. */
int evoamd_set_estep_counts(evoamd_ctx *ctx, double sum_nunique, double sum_sub);

/* ---- overlapping image patches (examples/image-denoising, image-inpainting: OverlappingPatches) ------ */
/* img (H, W, C) float64 row-major, C innermost (C = 1: grey).  Patch tops 0, s, 2s, ... while <= H - ph, plus H - ph
 * if that value was not reached (lefts alike with W, pw), so every pixel is covered; patch n = ir * nc + ic row-major
 * over the (top, left) grid, element d = (dy * pw + dx) * C + c, D = ph * pw * C.  Limits: ph * pw <= 1024, ph <= H,
 * pw <= W, shift >= 1 (else EVOAMD_E_INVALID).  Both calls take host pointers and have completed on return; they work
 * on an unconfigured context, use device scratch of their own (grown on demand, freed by evoamd_ctx_destroy) and
 * leave the EM state of a configured context (Y, K^n, Theta, masks, y_hat) untouched.
 * extract: Y_out (N, D) = the patches of img, NaN passed through. */
int evoamd_patches_extract(evoamd_ctx *ctx, const double *img, int H, int W, int C, int ph, int pw, int shift,
                           double *Y_out);
/* merge: Y (N, D) -> img_out (H, W, C), every element from the estimates of the patches that cover it, NaN skipped:
 * method 0 mean (summed in increasing n, divided by the count: np.nanmean of the NaN-padded estimate stack, bit for
 * bit), 1 median (np.nanmedian of that stack, bit for bit: even counts give (lo + hi) / 2).  No valid estimate: NaN. */
int evoamd_patches_merge(evoamd_ctx *ctx, const double *Y, int H, int W, int C, int ph, int pw, int shift, int method,
                         double *img_out);
/* precision-weighted merge: Y and V are (N, D) host arrays, the estimates and their variances;
 * img_out = (sum_k e_k w_k) / (sum_k w_k) with w_k = 1 / v_k over the covering patches in increasing n -- multiply and
 * add as separate IEEE operations (no contraction), both sums started from 0.0.  An estimate that is NaN, or whose v is
 * NaN or <= 0, is skipped; no valid estimate gives NaN.  evo_amd.utils.prepost.PrecisionMerger is the host mirror, bit
 * for bit.  Scratch and untouched state as for evoamd_patches_merge. */
int evoamd_patches_merge_weighted(evoamd_ctx *ctx, const double *Y, const double *V, int H, int W, int C, int ph, int pw,
                                  int shift, double *img_out);
/* The reconstruction without the N x D round trip: what Model.reconstruct / step(do_reconstruction) write into
 * my_data["y_reconstructed"] (_models.py:643-665) stays on the device and only the merged image comes back.
 * evoamd_reconstruct_resident makes the SELECTED reconstruction of the last statistics pass resident and copies nothing to
 * the host: y_rec[n, d] = keep(n, d) ? y[n, d] : y_hat[n, d], y_hat as evoamd_reconstruct forms it (same preconditions,
 * not in the float32 mode).  Incomplete data (evoamd_upload_masks): keep = x[n, d], or datapoint n has no reliable entry;
 * the masks on the device are used, the argument is not read, and the y_reconstructed that the statistics pass wrote for the
 * M-step (option "reconstruct_in_stats") is reused, not formed again.  A kept entry that is not reliable reads as NaN in the
 * merge (the device copy of Y holds a zero there, which the M-step keeps reading).  PRECONDITION for the merged image to
 * equal the merge of the host array: the caller's y is NaN wherever x_infr is 0, as in the examples; a finite value the
 * host keeps in such an entry is not on the device and cannot be merged from there.  Complete data:
 * x (N x D bool bytes) is the keep-mask, copied to the device by this call; NULL = every entry is estimated;
 * EVOAMD_KEEP_RESIDENT = the mask the previous call uploaded for this geometry (upload once per mask, not per epoch).
 * The resident reconstruction belongs to one statistics pass: the next pass, evoamd_set_params_*, evoamd_upload_data /
 * _masks / _yrec and evoamd_configure outdate it.
 * evoamd_patches_merge_resident: evoamd_patches_merge over it.  The patch geometry must give (N, D) of the configured
 * context; EVOAMD_E_INVALID when it does not or when no current resident reconstruction exists (never stale data).
 * Same kernels, same bits as evoamd_patches_merge of the host array; leaves the EM state untouched like it.  Option
 * "merge_select_fused" (default 0): a select kernel writes y_rec (NaN where a kept entry is not reliable) as N x D rows into
 * the patch scratch and the kernels of evoamd_patches_merge read that; 1: the merge kernels select while they gather (y,
 * y_hat and the masks read in place) -- one N x D write and read less, but measured slower.
 * evoamd_download_reconstruction: y_hat (N x D, host) of the resident reconstruction, for a caller that wants the array
 * after all; unlike evoamd_reconstruct it refuses (EVOAMD_E_INVALID) once the reconstruction is outdated. */
#define EVOAMD_KEEP_RESIDENT ((const uint8_t *)(uintptr_t)1)
int evoamd_reconstruct_resident(evoamd_ctx *ctx, const uint8_t *x_or_null);
int evoamd_patches_merge_resident(evoamd_ctx *ctx, int H, int W, int C, int ph, int pw, int shift, int method,
                                  double *img_out);
int evoamd_download_reconstruction(evoamd_ctx *ctx, double *y_hat);

/* ---- posterior code readout (the other product of a sparse-coding run: the code of each datapoint) ---- */
/* Both calls read the E_q rows the LAST statistics pass left on the device -- E_q[s_h] (both models) and E_q[s_h z_h]
 * (ES3C) per datapoint -- together with the K^n and lpj rows that pass read; they never run a pass themselves, and they
 * refuse (EVOAMD_E_INVALID, "call evoamd_stats first ...") once evoamd_set_params_*, a Theta update, an upload of data or
 * of K^n, or a K^n update has outdated the rows.  Not in the float32 mode.
 * evoamd_posterior_codes compacts the rows on the device (csrc/kernels_codes.hpp) and copies only the compact form:
 *   idx (N x max_active int32), p (N x max_active), m (N x max_active, ES3C; must be NULL for EBSC): the latents with
 *     E_q[s_h] > p_min by descending E_q[s_h], ties by ascending h, cut to max_active (1 .. 64); p = E_q[s_h],
 *     m = E_q[s_h z_h], both copied from the rows bit for bit; unused slots idx = -1, p = m = 0.  p_min >= 0.
 *   nnz (N int32): latents with E_q[s_h] > p_min BEFORE the cut (nnz > max_active: the code was truncated).
 *   map_slot (N int32): index of the largest entry of the lpj row (first one on ties; slots < S_perm are the permanent
 *     states), map_q (N): its posterior weight 1 / (sum_s exp(lpj_s - lpj_max) + tiny), map_state_packed
 *     (N x ceil(H/8) bytes): that state in np.packbits layout (evoamd_download_states_packed), the permanent all-zero
 *     state as zero bits.
 * Any output pointer may be NULL: that part is not copied.  Option "codes_path" (-1 automatic (default), 0 / 1 / 2): the
 * kernel keeps a datapoint's row in registers (H <= 512) / in LDS (H <= 4096) / re-reads it from memory (any H); same
 * results, for tests and measurements.
 * evoamd_download_posterior: the dense rows themselves, Es (N x H) and Ez (N x H, ES3C; NULL for EBSC), either may be
 * NULL -- 8 N H bytes each over PCIe where the codes are a few per cent of that. */
int evoamd_posterior_codes(evoamd_ctx *ctx, int max_active, double p_min, int32_t *idx, double *p, double *m,
                           int32_t *nnz, int32_t *map_slot, double *map_q, uint8_t *map_state_packed);
int evoamd_download_posterior(evoamd_ctx *ctx, double *Es, double *Ez);

/* ---- predictive uncertainty (posterior-predictive mean and variance of every entry) ---- */
/* evoamd_predictive_moments: for every datapoint n and observable d, reliable or missing, over the states s of K^n (and
 * the permanent all-zero state) with the weights q_ns = exp(lpj_ns - max) / (sum + tiny) of the statistics pass, read
 * from the lpj rows on the device:
 *   mean[n, d] = sum_s q_ns m_ns,d,   var[n, d] = sum_s q_ns ((m_ns,d - mean[n, d])^2 + v_ns,d) + (add_noise ? sigma^2 : 0)
 *   EBSC  m_ns = W s, v_ns = 0;   ES3C  m_ns = W_A kappa_ns, v_ns,d = w_dA^T Lam_ns w_dA with Lam_ns = (Psi_AA^-1 +
 *   W_oA^T W_oA / sigma2)^-1 and kappa_ns = mu_A + Lam_ns W_oA^T (y_o - W_oA mu_A) / sigma2 over the datapoint's reliable
 *   entries o (evoamd_upload_masks; all entries for complete data) -- `lam` and `lam_Wt` of sssc.py:289-303.
 * One wavefront per datapoint (csrc/kernels_predictive.hpp); the variance is accumulated in centred form (weighted
 * Welford), never as sum q m^2 - mean^2, and without the noise term it is never negative.  Every sum has a fixed order: a
 * call repeats bit for bit.  Runs no statistics pass and leaves K^n, lpj, Theta, y_reconstructed and the statistics rows
 * as they are (B = Y W is formed if it is not current, as by every lpj pass).  Needs data, K^n, lpj and Theta on the
 * device; not in the float32 mode.
 *   A datapoint without a reliable entry gets NaN rows and is counted in counters[1] (n_skipped).
 *   A datapoint with a singular k x k system -- an exactly zero or non-finite pivot of the partially pivoted elimination
 *   of Psi_AA or of I + Psi_AA G_A / sigma2, the criterion of the ES3C lpj levels -- among its states of non-zero weight
 *   gets NaN rows and is counted in counters[0] (n_singular).
 *   A state with more than 32 active latents (PRED_MAX_K): EVOAMD_E_INVALID naming the datapoint and k; nothing can be
 *   downloaded then.  D above 512 (64 lanes x 8 registers per lane): EVOAMD_E_INVALID before anything runs.
 * The results stay in device buffers of the context (grown on demand, freed by evoamd_ctx_destroy) until the next call;
 * evoamd_download_predictive copies mean and / or var (N x D double each; either may be NULL) to the host and refuses
 * (EVOAMD_E_INVALID) when the last call failed or the geometry has changed.  Both calls have completed on return. */
int evoamd_predictive_moments(evoamd_ctx *ctx, int add_noise, int64_t counters[2]);
int evoamd_download_predictive(evoamd_ctx *ctx, double *mean, double *var);

/* evoamd_predictive_score: the log predictive density and the PIT (the predictive CDF at the true value) of single entries
 * under the MIXTURE over K^n that evoamd_predictive_moments collapses to two moments (csrc/kernels_predictive_score.hpp has
 * the law; evo_amd.models.predictive_log_score_host is the NumPy mirror).  y_true (N x D double) and query (N x D bytes)
 * are host arrays; an entry is SCORED when its query byte is set and its y_true is finite; y_true is never read elsewhere.
 *   Weights e_s = exp(lpj_s - max lpj) in slot order (the permanent all-zero state first), a state of weight exactly 0 is
 *   skipped, Wsum = sum e_s; m_sd and v_sd per state exactly as evoamd_predictive_moments forms them (v clamped at 0).
 *   Per state and scored entry: tau = v_sd + (add_noise ? sigma^2 : 0), u = y_true - m_sd, ld = -(log(2 pi tau) + u^2 / tau) / 2,
 *   Phi = erfc(-u / sqrt(2 tau)) / 2; tau = 0 is a point mass: ld = -inf, Phi = [u >= 0].
 *   logp[n, d] = logsumexp_s((lpj_s - max lpj) + ld_s) - log Wsum, folded in slot order with a running maximum (-inf when
 *   no state has a density);  pit[n, d] = (sum_s e_s Phi_s) / Wsum.
 *   A queried entry with a non-finite y_true: NaN in logp and pit, left out of every sum and count, counted in counters[3].
 *   A datapoint without a scored entry is not visited (no decode, no solve): counters[2] (n_not_queried), logp_n 0, count 0.
 *   A datapoint without a reliable entry (counters[1], n_skipped) or with a singular system (counters[0], n_singular), as
 *   for evoamd_predictive_moments: NaN at every entry, logp_n 0, count 0.  Entries outside the query are NaN.
 * Outputs (host; out and each pointer may be NULL, logp and pit come together): logp, pit (N x D), logp_n (N; the sum of
 * the datapoint's scored entries), count (N; their number); total[2] = {the sum of logp_n, the sum of count}, reduced on
 * the device in a fixed order.  No atomics: two calls give the same bits.  Runs no statistics pass and leaves K^n, lpj,
 * Theta, the candidate batch, y_reconstructed, the statistics rows and the moments of evoamd_predictive_moments as they are
 * (B = Y W is formed if it is not current).  EVOAMD_E_INVALID, before anything is written: no data, Theta or K^n; the float32
 * mode; EBSC with add_noise = 0 (variance 0 everywhere); D above 512.  A state with more than 32 active latents in a VISITED
 * datapoint: EVOAMD_E_INVALID naming the datapoint and k; no output is written.  The call has completed on return. */
typedef struct evoamd_pred_score_out {
  double *logp;    /* (N, D) */
  double *pit;     /* (N, D) */
  double *logp_n;  /* (N) */
  int32_t *count;  /* (N) */
} evoamd_pred_score_out;
int evoamd_predictive_score(evoamd_ctx *ctx, const double *y_true, const uint8_t *query, int add_noise,
                            const evoamd_pred_score_out *out, int64_t counters[4], double total[2]);

/* ---- samples from the model (generate_data / generate_from_hidden: _models.py:73-99, bsc.py:27-57, sssc.py:66-102) ---- */
/* N datapoints drawn on the device, one wavefront each (csrc/kernels_generate.hpp):
 *   s_h ~ Bernoulli(pies[h]) (u <= pies[h]; EBSC: the caller fills pies with pi), or s given: s_packed (N x ceil(H/64)
 *     64-bit words, latent h in word h/64 at bit 63-(h%64), the device layout of K^n) is taken, not drawn;
 *   ES3C  z = s o (mus + F eps), eps ~ N(0, I_H), with F (H x H row-major) any matrix with F F^T = Psi -- the marginal on the
 *     active set A is N(mus_A, Psi_AA), the reference's law, without a factorisation per datapoint (evo_amd.models forms
 *     F = V sqrt(max(lambda, 0)) from eigh(Psi), which also serves a singular Psi);   EBSC  z = s, mus = F = NULL;
 *   y_mean = W z (Wt is W^T, H x D row-major),   y = y_mean + sigma g, g ~ N(0, I_D)   (ES3C: sigma = sqrt(sigma2)).
 * The stream is counter-based: datapoint n of the call is index first_index + n of the data set, so a set generated in
 * shards is the same set; s_h = rng_u01(seed, index, GEN_PURPOSE + 0, h) <= pies[h], eps_j / g_d = Box-Muller normal number
 * j / d of purpose GEN_PURPOSE + 1 / + 2 (kernels_generate.hpp has the definition; evo_amd.models.generate_counter is the
 * NumPy mirror: s bit for bit, the real-valued outputs to the last places of log / sincos).  Every sum has a fixed order:
 * a call repeats bit for bit.
 * keep: bits EVOAMD_GEN_KEEP_S | _Z | _YMEAN -- which outputs besides y are stored (z: ES3C only, the bit is ignored for
 * EBSC).  The outputs stay in device buffers of the context (grown on demand, freed by evoamd_ctx_destroy) until the next
 * evoamd_generate; evoamd_download_generated copies one to the host: what = EVOAMD_GEN_Y (N x D double), _S (N x ceil(H/64)
 * uint64), _Z (N x H double), _YMEAN (N x D double); EVOAMD_E_INVALID for an output the last call did not keep.
 * Needs no evoamd_configure and leaves the EM state of a configured context (Y, K^n, Theta, masks, lpj, statistics)
 * untouched.  H above 8192 (ES3C: the eps values of a datapoint no longer fit 64 KB of LDS) returns EVOAMD_E_INVALID.
 * Both calls have completed on return. */
enum { EVOAMD_GEN_KEEP_S = 1, EVOAMD_GEN_KEEP_Z = 2, EVOAMD_GEN_KEEP_YMEAN = 4 };
enum { EVOAMD_GEN_Y = 0, EVOAMD_GEN_S = 1, EVOAMD_GEN_Z = 2, EVOAMD_GEN_YMEAN = 3 };
int evoamd_generate(evoamd_ctx *ctx, int model, int64_t N, int D, int H, uint64_t seed, uint64_t first_index,
                    const double *Wt, const double *pies, const double *mus_or_null, const double *F_or_null, double sigma,
                    const uint64_t *s_packed_or_null, int keep);
int evoamd_download_generated(evoamd_ctx *ctx, int what, void *out);

/* ---- posterior samples (draws from q: states of K^n, ES3C latents, data rows) ---- */
/* evoamd_posterior_sample: for every datapoint n of the context and every draw t < n_samples, from the Theta, K^n and
 * lpj rows on the device (csrc/kernels_posterior_sample.hpp has the law; evo_amd.models.sample_posterior_counter is its
 * NumPy mirror: slot and s bit for bit, z and y to the rounding of the k x k arithmetic):
 *   slot  the column of lpj drawn with probability q_ns (0 .. S_perm + S - 1; the weights are those of
 *         evoamd_posterior_codes' map_q: a bit-reproducible exp, summed in slot order; a slot of weight 0 is never drawn);
 *   s     the drawn state: ceil(H/64) 64-bit words, latent h in word h/64 at bit 63-(h%64), all zero for the permanent
 *         all-zero state, the background unit set where that option is on;
 *   z     ES3C: z_A ~ N(kappa_s, Lam_s) on the active set with the Lam and kappa of evoamd_predictive_moments (Cholesky
 *         factor of the symmetrised Lam), 0 elsewhere;
 *   y     W z (EBSC: W s) + sigma g when add_noise; fill_all = 0: the reliable entries (evoamd_upload_masks; all of them
 *         for complete data) carry the datapoint's own y and only the others the draw; fill_all = 1: every entry the draw.
 * The stream is counter-based like evoamd_generate's, under a purpose of its own: datapoint n is index first_index + n of
 * the data set (shards concatenate to the single call) and draw t does not depend on n_samples (fewer draws are a prefix).
 * keep_mask: EVOAMD_PSAMP_KEEP_SLOT | _S | _Z | _Y -- only these outputs are allocated and written (z: ES3C only).
 * counters[4] = datapoints without draws (slot -1, s zero, z and y NaN in every row) because: [0] a drawn state has a
 * singular k x k system, [1] they have no reliable entry, [2] the Lam of a drawn state is not positive definite (an
 * indefinite Psi), [3] their lpj row holds a NaN or +inf or only -inf ("bad weights").  One wavefront per datapoint; every
 * sum has a fixed order and there are no atomics: a call repeats bit for bit.  Runs no statistics pass and leaves K^n, lpj,
 * Theta, y_reconstructed, the statistics rows and every validity flag of the EM state as they are (B = Y W is formed if
 * it is not current, as by every lpj pass).  Refusals (EVOAMD_E_INVALID): the float32 mode; D above 512; a state of K^n
 * with more than 32 active latents (the message names n and k; nothing can be downloaded then); outputs that do not fit
 * into the free device memory (the message names the bytes needed; decided before anything is launched).
 * The outputs stay in device buffers of the context (grown on demand, released by evoamd_configure and
 * evoamd_ctx_destroy) until the next call; evoamd_download_posterior_samples copies one to the host: what =
 * EVOAMD_PSAMP_SLOT (N x T int32), _S (N x T x ceil(H/64) uint64), _Z (N x T x H double), _Y (N x T x D double);
 * EVOAMD_E_INVALID for an output the last call did not keep.  Both calls have completed on return. */
enum { EVOAMD_PSAMP_KEEP_SLOT = 1, EVOAMD_PSAMP_KEEP_S = 2, EVOAMD_PSAMP_KEEP_Z = 4, EVOAMD_PSAMP_KEEP_Y = 8 };
enum { EVOAMD_PSAMP_SLOT = 0, EVOAMD_PSAMP_S = 1, EVOAMD_PSAMP_Z = 2, EVOAMD_PSAMP_Y = 3 };
int evoamd_posterior_sample(evoamd_ctx *ctx, int n_samples, uint64_t seed, uint64_t first_index, int keep_mask,
                            int fill_all, int add_noise, int64_t counters[4]);
int evoamd_download_posterior_samples(evoamd_ctx *ctx, int what, void *out);

/* ---- log-likelihood beyond K^n (importance draws from a proposal centred on q) ---- */
/* evoamd_loglik_estimate: for every datapoint n of the context, n_samples states drawn from a product of Bernoullis r_n
 * whose means are q_n's own marginals over K^n mixed with the prior (rho_h = (1 - prior_mix) p_h + prior_mix pi_h);
 * the draws K^n does not hold are evaluated by the model's lpj launches and folded onto the bound in the log domain:
 *   ll^_n = log( sum_{s in K^n} e^{lpj_ns} + (1 / T) sum_t 1[s_t not in K^n] e^{lpj(s_t)} / r_n(s_t) ).
 * Unbiased in the likelihood, ll^_n >= F_n for every datapoint and seed, E[ll^_n] <= log p(y_n) - ljc.
 * csrc/kernels_loglik_estimate.hpp has the law; evo_amd.models.estimate_log_likelihood_counter is its NumPy mirror (the
 * draws, inside / outside and n_outside bit for bit, the real values to rounding).  The stream is counter-based under a
 * purpose of its own: datapoint n is index first_index + n of the data set (shards concatenate to the single call) and
 * draw t depends neither on n_samples nor on the passes (fewer draws are a prefix).
 * Outputs (host, N each, any may be NULL): ll_out = ll^_n without ljc; F_out = the bound, evoamd_posterior_scores' F;
 * mass_out = the share of Z^_n from outside K^n; ess_out = (sum w)^2 / sum w^2 over the outside draws; n_outside_out
 * (int32).  sum_out (required) = sum of ll^_n over the datapoints that have an estimate.  counters[2] = datapoints without
 * one (NaN outputs, left out of the sum) because [0] their lpj row holds a NaN or +inf or only -inf ("bad weights"), [1]
 * they have no reliable entry.
 * The draws run in passes of Cmax (the configured candidate capacity) through the resident candidate buffers and the
 * candidate lpj launches: on return NO candidate batch counts as installed (evoamd_vary_kn refuses until the next
 * evoamd_lpj_candidates / evolve call).  K^n, lpj, Theta, the statistics rows, y_reconstructed, a prefetched pass and the
 * reset counters the next evoamd_stats reports stay as they are (the draws' clamp flags go to words of the call's own).
 * The first pass leaves the proposal (N x 64 KH doubles, KH = the power of two >= ceil(H/64)) and one hash per state of
 * K^n (N x S words) in buffers of the context for the later passes (grown on demand, released by evoamd_configure).
 * keep_draws != 0: the draws stay in device buffers of the context (grown on demand, released by evoamd_configure and
 * evoamd_ctx_destroy) for evoamd_download_loglik_draws: what = EVOAMD_LLE_S (N x T x ceil(H/64) uint64, the layout of
 * K^n), _INSIDE (N x T uint8), _LOG_R (N x T double), _LPJ (N x T double, NaN where the draw is inside K^n).
 * Refusals (EVOAMD_E_INVALID) before anything is launched: n_samples < 1; prior_mix outside (0, 1]; the float32 mode;
 * H above 1024 (64 lanes x 16 latents per lane); S_perm + 2 S above 2048 (the weights and state hashes of a datapoint
 * live in LDS); buffers that do not fit into the free device memory (the message names the bytes).  ES3C: a draw the lpj
 * levels refuse surfaces as EVOAMD_E_KLIMIT / EVOAMD_E_SINGULAR, as for evoamd_lpj_candidates.  Both calls have completed
 * on return. */
enum { EVOAMD_LLE_S = 0, EVOAMD_LLE_INSIDE = 1, EVOAMD_LLE_LOG_R = 2, EVOAMD_LLE_LPJ = 3 };
int evoamd_loglik_estimate(evoamd_ctx *ctx, int n_samples, uint64_t seed, uint64_t first_index, double prior_mix,
                           int keep_draws, double *ll_out, double *F_out, double *mass_out, double *ess_out,
                           int32_t *n_outside_out, int64_t counters[2], double *sum_out);
int evoamd_download_loglik_draws(evoamd_ctx *ctx, int what, void *out);

/* ---- merges of the resident draws and predictive moments (nothing of N x T x D or N x D crosses to the host) ---- */
/* The patch geometry (H, W, C, ph, pw, shift: the conventions of evoamd_patches_merge) must give (N, D) of the buffers.
 * evoamd_patches_merge_samples merges draws t0 .. t0+n_draws-1 of the y draws the last evoamd_posterior_sample kept, each
 * draw t read where it lies (element ((n T + t) D + d)), in one launch per method:
 *   imgs_out  (n_draws, H, W, C) or NULL: image t is, bit for bit, evoamd_patches_merge of the dense slice y[:, t, :]
 *             (method 0 mean, 1 median; estimates in increasing n, NaN skipped, no valid estimate gives NaN);
 *   mean_out / std_out  (H, W, C) or NULL: the pixelwise moments over those merged images, in draw order, by Welford from
 *             mean = 0, M2 = 0: delta = x_t - mean, mean += delta / t, M2 += delta (x_t - mean), as separate IEEE
 *             operations; mean_out = mean, std_out = sqrt(M2 / n_draws) (ddof 0).  A NaN in any image makes both NaN at
 *             that pixel; identical images give their value and exactly 0.  evo_amd.utils.prepost.image_moments_host is
 *             the NumPy mirror, bit for bit.  With method 0 the images are not stored when imgs_out is NULL.
 * evoamd_patches_merge_predictive merges the mean / var buffers of the last evoamd_predictive_moments: what = 0 mean-merge
 * of mean, 1 median-merge of mean, 2 precision-weighted merge of mean by var (evoamd_patches_merge_weighted), 3 mean-merge
 * of var (the per-pixel uncertainty map) -- the kernels of evoamd_patches_merge / _weighted reading the context's buffers,
 * hence their bits.
 * Both refuse with EVOAMD_E_INVALID before anything is launched: a geometry that does not give (N, D) of the buffers; t0 or
 * n_draws outside the T of the last call (n_draws 1 .. 65535); y not kept; no current results (the last sample / predictive
 * call failed, or evoamd_configure released them: never stale data); for samples, imgs_out, mean_out and std_out all NULL.
 * Both leave the EM state and every validity flag as they are, put the images into the context's patch scratch (grown on
 * demand: n_draws + 2 images at most), allocate nothing of the size of the draws, and have completed on return. */
int evoamd_patches_merge_samples(evoamd_ctx *ctx, int H, int W, int C, int ph, int pw, int shift, int method,
                                 int t0, int n_draws, double *imgs_out, double *mean_out, double *std_out);
int evoamd_patches_merge_predictive(evoamd_ctx *ctx, int H, int W, int C, int ph, int pw, int shift, int what,
                                    double *img_out);

/* ---- the dictionary resized: prune, reorder, grow ------------------------------------ */
/* K^n moved to a new latent numbering on the device (csrc/kernels_remap.hpp has the law;
 * evo_amd.variational.remap_states_host is its NumPy mirror, bit for bit).  index: int32 (H_new); an entry >= 0 names a
 * source latent in [0, H), each at most once; -1 marks a NEW latent, off in every state.  Hv' = H_new - 1 with the
 * "background_unit" option (the last entry must then be H - 1: the unit stays last and on), else H_new.  Per datapoint:
 *   gather  t_j[h'] = s_j[index[h']] where index[h'] >= 0, else 0, for the S slots of K^n (the permanent all-zero column of
 *           S_perm = 1 is not a slot);
 *   keep    slot j is kept iff t_j differs from every t_i with i < j and, where S_perm = 1, is not the all-zero state;
 *   fill    the other slots, in ascending order, each take the next state of the enumeration {0}, {1}, .. {Hv' - 1}, {0,1},
 *           {0,2}, .. {0,Hv'-1}, {1,2}, .. (each ORed with the background bit) that equals no kept state of the datapoint;
 *   bound   Hv' (Hv' + 1) / 2 >= S, so that the enumeration cannot run out.
 * The result -- packed states (N, S, ceil(H_new/64)), their digests, n_replaced (N) -- goes to scratch the context owns and
 * that survives evoamd_configure; the resident K^n, the lpj rows and every validity flag stay as they are.
 * n_replaced_out (N) and sum_out may be NULL.  Deterministic: two calls give the same bits.
 * EVOAMD_E_INVALID, before anything is launched and with the context as it was, for: no configured context or a K^n lost
 * to a failed evoamd_init_states; an index entry outside {-1} + [0, H); a source named twice; with the background unit a
 * last entry other than H - 1; H_new outside [1, 16384]; the bound; and an S whose LDS slice -- 8 S (ceil(H/64) +
 * ceil(H_new/64) + 1) bytes beside 256 ceil(H_new/64) bytes of index -- exceeds 150 KiB (S <= 1024 fits up to
 * H + H_new = 1088; the message names the cap of the shape).
 * Then: evoamd_configure for H_new (same N and S), data and Theta as usual, and evoamd_adopt_remapped_states, which makes
 * the scratch the resident K^n and digests -- what evoamd_upload_states of the same rows leaves, with the same
 * invalidations (census, row statistics, prefetched pass) -- and releases it.  EVOAMD_E_INVALID with K^n as it was when
 * (N, S, H) of the context differ from the scratch's, and for an adopt without a remap before it (a second adopt). */
int evoamd_remap_latents(evoamd_ctx *ctx, const int32_t *index, int H_new, int32_t *n_replaced_out, int64_t *sum_out);
int evoamd_adopt_remapped_states(evoamd_ctx *ctx);
/* ---- K^n resized: S changes, the best states stay, new slots are filled near the best -- */
/* (csrc/kernels_resize.hpp has the law; evo_amd.variational.resize_states_host is its NumPy mirror, bit for bit.)  Per
 * datapoint, independently, from the S varying slots of the resident K^n and the datapoint's lpj row (the permanent all-zero
 * column of S_perm = 1 is not a slot and is carried over untouched); Hv = H - 1 with the "background_unit" option, else H:
 *   keys    slot j has key seed_key(lpj[n, S_perm + j]): NaN and +-inf rank as -inf, -0 equals +0.  Rank order is
 *           descending key, then ascending slot.
 *   shrink  (S_new < S) the kept slots are the first S_new in rank order, written in ascending old slot (a stable
 *           compaction); src_slot[n, j'] is the old slot of new slot j'.
 *   grow    (S_new > S) slots 0 .. S - 1 are copied in place, src_slot[n, j] = j.  With b the best varying state (rank 0)
 *           and e_c candidate c of the enumeration {0}, .. {Hv - 1}, {0,1}, {0,2}, .. {Hv-2, Hv-1}, the candidate fill is
 *           f_c = b XOR e_c: the one-flip neighbours of the best state in ascending latent, then its two-flip neighbours.
 *           f_c is skipped when it has no varying latent on or equals (on the full words) a state the datapoint holds.
 *           Slots S, S + 1, .. take the unskipped f_c in ascending c; src_slot is -1 there.  The background bit stays on.
 *   bound   Hv (Hv + 1) / 2 - 1 >= S_new on a grow, so that the enumeration cannot run out.
 * The result -- packed states (N, S_new, ceil(H/64)), their digests, src_slot int32 (N, S_new) -- goes to scratch the context
 * owns and that survives evoamd_configure; the resident K^n, the lpj rows and every validity flag stay as they are.
 * src_slot_out (N * S_new) may be NULL.  No floating point beyond the key, no random numbers, no atomics: two calls give the
 * same bits.  EVOAMD_E_INVALID, before anything is launched or allocated and with the context as it was, for: no configured
 * context or a K^n lost to a failed evoamd_init_states; lpj rows that are not those of the resident K^n (evoamd_lpj_resident,
 * an E-step or evoamd_upload_lpj after the last change of K^n by the caller makes them so); S_new < 1, S_new = S, S or
 * S_new above 1024; H above 16384; the bound; a share of LDS -- 8 (S + ceil(H/64)) + 4 S_new bytes -- above 150 KiB (no
 * admitted shape reaches it); scratch that does not fit the free device memory.
 * Then: evoamd_configure for (N, H, S_new), data and Theta as usual, and evoamd_adopt_resized_states, which makes the scratch
 * the resident K^n and digests -- what evoamd_upload_states of the same rows leaves, with the same invalidations -- and
 * releases it.  EVOAMD_E_INVALID with K^n as it was when (N, S, H) of the context differ from the scratch's, and for an
 * adopt without a resize before it (a second adopt). */
int evoamd_resize_states(evoamd_ctx *ctx, int S_new, int32_t *src_slot_out);
int evoamd_adopt_resized_states(evoamd_ctx *ctx);
/* counts_out (H): the number of datapoints whose most probable state of K^n -- the first column of maximal lpj, the rule of
 * evoamd_posterior_scores' best -- has latent h on.  Integer atomics: independent of the order.  Needs valid lpj rows;
 * nothing of the EM state changes. */
int evoamd_latent_map_counts(evoamd_ctx *ctx, int64_t *counts_out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------------- */
/* 128-byte opaque id made by rank 0 and distributed by the caller (file / socket / MPI). */
int evoamd_comm_unique_id(uint8_t id_out[128]);
int evoamd_comm_init(evoamd_ctx *ctx, const uint8_t id[128], int rank, int world);
/* In-place sum / max all-reduce of a small host double vector through the device
 * (used for barriers and max-over-ranks timing). op: 0 sum, 1 max. */
int evoamd_comm_allreduce_host(evoamd_ctx *ctx, double *buf, int64_t n, int op);
int evoamd_comm_destroy(evoamd_ctx *ctx);

/* ---- timing (HIP events on the context's stream) ------------------------------------ */
/* Kernel-class ids for evoamd_kernel_time_ms: average device time per launch since the last
 * evoamd_timing_reset, measured with hipEvents recorded on the stream the kernels run on. */
enum {
  EVOAMD_K_LPJ_RESIDENT = 0,   /* main lpj kernel on K^n (N x S): bsc_lpj_gram2_kernel / sssc_main_lpj_kernel (|s| <= 2) */
  EVOAMD_K_LPJ_CANDIDATES = 1, /* main lpj kernel on the candidate batch                                                  */
  EVOAMD_K_LPJ_OVERFLOW = 2,   /* ES3C states with |s| > 2: K=4 / K=8 register kernels + LDS wavefront kernel (any batch)   */
  EVOAMD_K_ROW_LSE = 3,        /* free energy / posterior normalisers when vary_kn did not leave them behind              */
  EVOAMD_K_VARY_KN = 4,
  EVOAMD_K_STATS = 5,          /* bsc_stats_wave_kernel / sssc_stats_wave_kernel (|s| <= 2) + pair_bins_reduce_kernel      */
  EVOAMD_K_STATS_OVERFLOW = 6, /* ES3C statistics of the states with |s| > 2                                              */
  EVOAMD_K_GEMM = 7,           /* f64 MFMA contractions                                     */
  EVOAMD_K_EVOLVE = 8,
  EVOAMD_K_MISC = 9,
  EVOAMD_K_MSTEP_DEVICE = 10,  /* device Theta update (inverse, GEMMs, precompute) */
  EVOAMD_K_LPJ_PASS = 11,      /* whole pass over the resident K^n: main kernel + every overflow level (one span) */
  EVOAMD_K_STATS_PASS = 12,    /* whole statistics pass: scatter + overflow levels + bin reduce + finish, GEMM aside */
  EVOAMD_K_LPJ_K3_4 = 13,      /* ES3C census levels of the pass over K^n: states with 3..4 active latents (sssc_quad_kernel<1>), */
  EVOAMD_K_LPJ_K5_8 = 14,      /* 5..8 (sssc_quad_kernel<2>),                                                                    */
  EVOAMD_K_LPJ_K9PLUS = 15,    /* more than 8, or handed on by a quad kernel (pivoting wavefront kernel)                          */
  EVOAMD_K_STATS_K3_4 = 16,    /* the same levels of the statistics pass */
  EVOAMD_K_STATS_K5_8 = 17,
  EVOAMD_K_STATS_K9PLUS = 18,
  EVOAMD_K_ALLREDUCE = 19,     /* RCCL all-reduce(s) of the packed accumulator (sssc.py:671-691 / bsc.py:230-274 in one call): from
                                  this rank's statistics being done to the sum being delivered, i.e. wait for the slowest rank + transfer */
  EVOAMD_K_ESTEP_FUSED = 20,   /* fused per-datapoint E-step kernel (option "fused_estep") */
  EVOAMD_K_PATCHES = 21,       /* evoamd_patches_extract / evoamd_patches_merge kernels (transfers excluded) */
  EVOAMD_K_INIT_STATES = 22,   /* evoamd_init_states: the K^n(0) sampler */
  EVOAMD_K_POSTERIOR_SAMPLE = 23, /* evoamd_posterior_sample: W^T and the sampling kernel (transfers excluded) */
  EVOAMD_K_SEED_STATES = 24,   /* evoamd_seed_states: the greedy K^n seeding kernel (B = Y W and transfers excluded) */
  EVOAMD_K_LOGLIK_PROPOSAL = 25, /* evoamd_loglik_estimate: the proposal kernel (marginals, draws, membership), per pass */
  EVOAMD_K_LOGLIK_LPJ = 26,    /* ... the lpj launches over a pass's outside draws (every level)                          */
  EVOAMD_K_LOGLIK_FOLD = 27,   /* ... the fold kernel of a pass; the bound + all-zero terms and the finish (one span each) */
  EVOAMD_K_REMAP = 28,         /* evoamd_remap_latents: the remap kernel (index upload and downloads excluded) */
  EVOAMD_K_STATS_KAPPA = 29,   /* the ES3C statistics kernel on the kappa route (option "stats_kappa"), nested in EVOAMD_K_STATS */
  EVOAMD_K_SWEEP = 30,         /* evoamd_sweep_propose / evoamd_sweep_states: the proposal kernel (ES3C: with the transpose of GP) */
  EVOAMD_K_SWEEP_SWAP = 31,    /* evoamd_sweep_*_nb with EVOAMD_SWEEP_SWAP: the swap proposal kernel */
  EVOAMD_K_RESIZE = 32,        /* evoamd_resize_states: the resize kernel (downloads excluded) */
  EVOAMD_K_NBOUND = 33,        /* evoamd_neighbour_bound: the neighbourhood kernel (ES3C: with the transpose of GP) and the bound of the rows */
  EVOAMD_K_PRED_SCORE = 34,    /* evoamd_predictive_score: the transpose of W, the visit list, the score kernel, its partials and their reductions */
  EVOAMD_K_AIS = 35,           /* evoamd_ais_loglik: the chain kernel, the fold over the chains and (admit) the emission */
  EVOAMD_K_AIS_POST = 36,      /* evoamd_ais_posterior: the chain kernel and the fold of every block of datapoints (the product for mean counts as gemm); _sel: the emission and the tally too */
  EVOAMD_K_COUNT = 37
};
/* on = bit mask of kernel classes to time (bit k = class k; -1 = all, 0 = off).  Each timed span
 * records two HIP events on the compute stream, which costs about 10 us of stream time per span:
 * a throughput run times only the class it needs. */
int evoamd_timing_enable(evoamd_ctx *ctx, int on);
/* the same with a 64-bit mask: the classes from 32 on have no bit in the int (which reaches them with -1 only) */
int evoamd_timing_enable64(evoamd_ctx *ctx, uint64_t on);
int evoamd_timing_reset(evoamd_ctx *ctx);
int evoamd_kernel_time_ms(evoamd_ctx *ctx, int kernel_class, double *avg_ms, int64_t *launches);
const char *evoamd_kernel_name(int kernel_class);

#ifdef __cplusplus
}
#endif
#endif /* EVO_AMD_H */
