// libevo_amd.so -- C ABI (include/evo_amd.h) over the gfx950 kernels.
// Host side of the library: context, device memory, launch geometry, RCCL, timing.
#include "../../include/evo_amd.h"

#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "gemm_f64.hpp"
#include "kernels_bsc.hpp"
#include "kernels_common.hpp"
#include "kernels_evolve.hpp"
#include "kernels_mstep.hpp"
#include "kernels_sssc.hpp"
#include "kernels_sssc_quad.hpp"
#include "kernels_fused.hpp"
#include "kernels_patches.hpp"
#include "kernels_codes.hpp"
#include "kernels_init.hpp"
#include "kernels_generate.hpp"
#include "kernels_exact.hpp"
#include "kernels_predictive.hpp"
#include "kernels_predictive_score.hpp"
#include "kernels_posterior_sample.hpp"
#include "kernels_seed.hpp"
#include "kernels_seed_beam.hpp"
#include "kernels_refine.hpp"
#include "kernels_loglik_estimate.hpp"
#include "kernels_remap.hpp"
#include "kernels_resize.hpp"
#include "kernels_sweep.hpp"
#include "kernels_sweep_swap.hpp"
#include "kernels_nbound.hpp"
#include "kernels_ais.hpp"
#include "kernels_ais_post.hpp"

// ---------------------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(EVOAMD_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                  __LINE__);                                                                   \
  } while (0)

// EVOAMD_DEBUG_SYNC=1: synchronise after every launch group and say which one on stderr, so that a GPU fault
// (the runtime aborts the process at the next synchronisation) is attributed to the kernel that caused it.
static const bool g_dbg_sync = getenv("EVOAMD_DEBUG_SYNC") != nullptr;
#define DBG_SYNC(c, what)                                                    \
  do {                                                                       \
    if (g_dbg_sync) {                                                        \
      fprintf(stderr, "[evoamd] %s ...", what);                              \
      fflush(stderr);                                                        \
      hipError_t _de = hipStreamSynchronize((c)->stream);                    \
      fprintf(stderr, " %s\n", hipGetErrorString(_de));                      \
      fflush(stderr);                                                        \
    }                                                                        \
  } while (0)

#define REQUIRE(cond, msg)                                   \
  do {                                                       \
    if (!(cond)) return fail(EVOAMD_E_INVALID, "%s", msg);   \
  } while (0)
// After a failed evoamd_init_states (kn_lost) K^n is partly written.  Guarded directly: the downloads of K^n, lpj_resident,
// vary_kn, evolve_randflip, estep, evolve_states and the statistics pass (hence mstep_device and the pass it prefetches);
// posterior_codes refuses through kn_gen (the failed call bumps it, so the rows of the last pass are outdated).  Nothing
// else reads c->states / c->dig: lpj_candidates, set_candidates, lpj_shared, lpj_single and the reconstruction calls work on
// the candidate batch, on states the caller passes or on the rows of the last statistics pass.
#define REQUIRE_KN(c) \
  REQUIRE(!(c)->kn_lost, "K^n is not on the device: evoamd_init_states stopped at its round cap (upload or initialise K^n first)")

// ---------------------------------------------------------------------------------------
// RCCL through dlopen (so the library loads on hosts without librccl)
// ---------------------------------------------------------------------------------------
struct RcclId {
  char internal[128];
};
struct RcclApi {
  void *handle = nullptr;
  int (*GetUniqueId)(RcclId *) = nullptr;
  int (*CommInitRank)(void **, int, RcclId, int) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;

static int rccl_load() {
  if (g_rccl.handle) return 0;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *nm : names) {
    h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
  }
  if (!h) return fail(EVOAMD_E_RCCL, "cannot dlopen librccl: %s", dlerror());
  g_rccl.GetUniqueId = (int (*)(RcclId *))dlsym(h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void **, int, RcclId, int))dlsym(h, "ncclCommInitRank");
  g_rccl.AllReduce =
      (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclAllReduce");
  g_rccl.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
  g_rccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
    return fail(EVOAMD_E_RCCL, "librccl is missing a required symbol");
  g_rccl.handle = h;
  return 0;
}
#define RCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    int _r = (expr);                                                                           \
    if (_r != 0)                                                                               \
      return fail(EVOAMD_E_RCCL, "%s failed: %s", #expr,                                       \
                  g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "?");                    \
  } while (0)

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
enum {  // internal kernel ids (see evoamd_kernel_name)
  KID_LPJ_RES = 0,
  KID_LPJ_CAND,
  KID_LPJ_OVF,
  KID_ROW_LSE,
  KID_VARY_KN,
  KID_STATS,
  KID_STATS_OVF,
  KID_GEMM,
  KID_EVOLVE,
  KID_MISC,
  KID_MSTEP,
  KID_LPJ_PASS,    // the whole pass over the resident K^n: main kernel + every overflow level it spawns
  KID_STATS_PASS,  // the whole statistics pass: scatter kernels + overflow levels + column sums + finish (no GEMM)
  KID_LPJ_K34,     // census levels of the pass over K^n: states with 3..4 / 5..8 / more than 8 active latents
  KID_LPJ_K58,
  KID_LPJ_K9P,
  KID_STATS_K34,   // ... and of the statistics pass
  KID_STATS_K58,
  KID_STATS_K9P,
  KID_ALLREDUCE,    // the RCCL all-reduce(s) of the packed accumulator: local statistics done -> sum delivered
  KID_ESTEP_FUSED,  // the fused per-datapoint E-step kernel (lpj of K^n -> candidates -> their lpj -> vary_Kn -> census)
  KID_PATCHES,      // overlapping image patches: extract / mean merge / median merge kernels
  KID_INIT_STATES,  // evoamd_init_states: the K^n(0) sampler (or the table copy of the exact mode)
  KID_POSTERIOR_SAMPLE,  // evoamd_posterior_sample: W^T and the sampling kernel (transfers excluded)
  KID_SEED_STATES,  // evoamd_seed_states: the greedy seeding kernel
  KID_LLE_PROPOSAL,  // evoamd_loglik_estimate: the proposal kernel (marginals, draws, membership), all passes
  KID_LLE_LPJ,       // ... the lpj launches over the outside draws, all passes
  KID_LLE_FOLD,      // ... the fold kernel of every pass and the finish
  KID_REMAP,         // evoamd_remap_latents: the remap kernel (index upload and downloads excluded)
  KID_STATS_KAPPA,   // the ES3C statistics kernel on the kappa route (option "stats_kappa"), nested in KID_STATS: its launch count
                     // says which route a pass took
  KID_SWEEP,         // evoamd_sweep_propose / evoamd_sweep_states: the proposal kernel (ES3C: with the transpose of GP)
  KID_SWEEP_SWAP,    // evoamd_sweep_*_nb with EVOAMD_SWEEP_SWAP: the swap proposal kernel
  KID_RESIZE,        // evoamd_resize_states: the resize kernel (downloads excluded)
  KID_NBOUND,        // evoamd_neighbour_bound: the neighbourhood kernel (ES3C: with the transpose of GP) and the bound of the rows
  KID_PRED_SCORE,    // evoamd_predictive_score: the transpose of W, the visit list, the score kernel, its partials and their two reductions
  KID_AIS,           // evoamd_ais_loglik: the chain kernel and the fold over the chains (admit: the emission; its lpj and selection count in their own classes)
  KID_AIS_POST,      // evoamd_ais_posterior: the chain kernel and the fold of every block of datapoints (the product for `mean` counts as gemm); _sel: the emission and the tally too
  KID_COUNT
};

struct TimedSpan {
  hipEvent_t a, b;
  int kid;
};

// ---------------------------------------------------------------------------------------
// owning buffers (DESIGN: buffer ownership).  The only hipMalloc / hipHostMalloc / hipFree / hipHostFree of the library.
// ---------------------------------------------------------------------------------------
static int sync_streams(evoamd_ctx *c);
static std::atomic<int64_t> g_live_dev{0}, g_live_pinned{0};  // evoamd_debug_live_buffers

// Device memory of n elements of T.  Converts to T* so that launches and copies read as before; a kernel template that
// deduces its element type from the argument takes get().
template <typename T>
class DevBuf {
  T *p_ = nullptr;
  size_t n_ = 0;

  hipError_t alloc_raw(size_t n) {
    reset();
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    n_ = n;
    g_live_dev++;
    return hipSuccess;
  }

 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T *() const { return p_; }
  T *get() const { return p_; }
  size_t size() const { return n_; }  // elements; 0 = empty
  void reset() {
    if (p_) {
      (void)hipFree(p_);
      g_live_dev--;
    }
    p_ = nullptr;
    n_ = 0;
  }
  // exactly n elements (0 becomes 1), whatever was there before is freed first; on failure the buffer is empty
  int alloc(size_t n) {
    hipError_t e = alloc_raw(n);
    if (e != hipSuccess) return fail(EVOAMD_E_HIP, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    return 0;
  }
  // the optional buffers: false (and no sticky HIP error) when the memory cannot be had
  bool try_alloc(size_t n) {
    if (alloc_raw(n) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  // grow-only: nothing but a compare while n fits; else wait for whatever may still read the old buffer and re-cut
  int ensure(evoamd_ctx *c, size_t n) {
    if (n <= n_) return 0;
    int r = sync_streams(c);
    return r ? r : alloc(n);
  }
};

// hipHostMalloc memory of n elements of T.
template <typename T>
class PinnedBuf {
  T *p_ = nullptr;
  size_t n_ = 0;

 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  PinnedBuf &operator=(PinnedBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  operator T *() const { return p_; }
  T *get() const { return p_; }
  size_t size() const { return n_; }
  void reset() {
    if (p_) {
      (void)hipHostFree(p_);
      g_live_pinned--;
    }
    p_ = nullptr;
    n_ = 0;
  }
  int alloc(size_t n, unsigned flags = hipHostMallocDefault) {
    reset();
    if (n == 0) n = 1;
    hipError_t e = hipHostMalloc((void **)&p_, n * sizeof(T), flags);
    if (e != hipSuccess) {
      p_ = nullptr;
      return fail(EVOAMD_E_HIP, "hipHostMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    }
    n_ = n;
    g_live_pinned++;
    return 0;
  }
};

#define TRY(expr)        \
  do {                   \
    int _r = (expr);     \
    if (_r) return _r;   \
  } while (0)

// The buffers a call is about to size, each named once.  Asked before anything is released, allocated or launched: they fit
// unless grow > avail; the refusal and its hint are the caller's.  ensure_all() then grows them in the order listed.
struct FitList {
  size_t grow = 0, released = 0;  // bytes of the buffers that must grow; bytes those give back when they are re-cut
  std::vector<std::function<int(evoamd_ctx *)>> ensures;
  template <typename T>
  void add(DevBuf<T> &b, size_t want) {
    if (want > b.size()) grow += want * sizeof(T), released += b.size() * sizeof(T);
    ensures.push_back([&b, want](evoamd_ctx *c) { return b.ensure(c, want); });
  }
  int measure(size_t &avail) const {  // avail: the free device memory plus `released` (no query while nothing grows)
    size_t free_b = 0, total_b = 0;
    if (grow) HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    avail = free_b + released;
    return 0;
  }
  int ensure_all(evoamd_ctx *c) const {
    for (const auto &e : ensures) TRY(e(c));
    return 0;
  }
};

struct evoamd_ctx {
  evoamd_ctx() = default;
  evoamd_ctx(const evoamd_ctx &) = delete;
  evoamd_ctx &operator=(const evoamd_ctx &) = delete;
  ~evoamd_ctx();  // releases the streams, the events and the communicator; the buffers release themselves
  int device = 0;
  hipStream_t stream = nullptr;
  // second stream: the K = N statistics contraction runs beside the H x H elimination chain of the
  // Theta update (independent inputs; the chain is launch-latency bound, the GEMM MFMA bound)
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool gemm_forked = false;
  // Theta^new reaches the host through the copy engine (third stream) while the kernels of the refresh and of the
  // prefetched pass run: the mailbox kernel then carries the 32-word header only (it used to write the 3 MB of Theta
  // into pinned memory itself: 67 us in front of everything queued behind it).  Option "theta_copy_engine" = 0: old form.
  hipStream_t stream_copy = nullptr;
  hipEvent_t ev_theta = nullptr, ev_theta_done = nullptr;
  hipEvent_t ev_mbox = nullptr, ev_bak = nullptr;  // mailbox kernel / Theta backup on the side stream (off the critical path)
  int mbox_side = 1;  // option "mailbox_side_stream"
  int theta_copy_engine = 0;  // measured (c4 / c4shard, interleaved A/B): no gain -- the host then waits for the copy
                              // instead, and at N / 8 it returns too late to keep the queue filled (1.30 vs 1.25 ms)
  double rel_frac = -1.0;  // EBSC incomplete data: sum(x_infr) / N over all ranks (evoamd_set_reliable_fraction)
  bool ar_gemm_pending = false;  // with a communicator: the contraction's block of acc is all-reduced at the join
  int overlap_gemm = 1;  // option "overlap_gemm": 0 never, 1 where it was measured to pay, 2 always
  // option "early_fork": the forked contraction needs the [Es | Ez] rows only, so its stream may branch off BEFORE the
  // pair-bin reduce and the finish kernel (which complete the H x H sums for the Theta chain) instead of behind them
  // (-1 = automatic: products below 2e10 flops -- c2 0.377 -> 0.368 ms per iteration together with the fork itself, which
  // alone costs 11 us there; N / 8 of c4 1.122 -> 1.114; N / 4 and larger lose 2-5 %: the persistent product then takes the
  // slots the reduce needs)
  int early_fork = -1;
  // option "background_unit" (permanent["background"], variational/utils.py:42-47): the last latent is on in every state;
  // the evolutionary operators leave it alone (eas.py:213-239) and the Theta update pins its prior to 1 - 1.1e-5
  // (bsc.py:259-260, sssc.py:718-719)
  int bg_unit = 0;
  // option "fold_clear": evoamd_vary_kn's kernel zeroes the accumulators of the next statistics pass and checks + clears
  // the census counters on its way (was a memset and a one-workgroup kernel in front of the census)
  int fold_clear = 1;
  bool acc_clean = false, clist_clean = false;
  bool wq_copy_valid = false;  // EBSC: tmpA holds a copy of Wq (written by the finish kernel of the last statistics pass)
  int stats_chunks = 1;  // option "stats_chunks": the statistics pass runs in this many blocks of datapoints, the MFMA
                         // contraction of block i on the second stream beside the scatter kernels of block i + 1.
                         // Measured at the north-star shape (N = 100k, H = 512): 1 block 5.47 ms per iteration, 2 blocks
                         // 5.61, 4 blocks 5.68-5.88, 8 blocks 5.99 -- both kernels live on the memory-side f64 atomic
                         // units (the contraction's split-K epilogue issues 36 M of them) and they time-slice the CUs
                         // instead of overlapping; off by default
  // ES3C pair bins (kernels_sssc.hpp: PairBins): option "pair_bins" 0 never / 1 when the flush is a small part of
  // the contributions / 2 always
  int n_cu = 256;  // compute units of the device (persistent grids)
  int stats_stage = 1;  // option "stats_stage" (measurement): 0 = no LDS staging of B rows / singleton table
  int stats_waves = 0;  // option "stats_waves" (measurement): waves per workgroup of the ES3C statistics kernel, 0 = 4
  PairBins pbins = {};  // views into the three buffers below (alloc_pair_bins), all null when the bins do not fit
  DevBuf<double4> pb_ent;
  DevBuf<double> pb_part;
  DevBuf<int> pb_gcnt;
  int bins_min = 256;  // option "pair_bins_min": pair bins from this many resident states (x 1024) on
 int bins_scale = 3;  // option "pair_bins_scale" (read by evoamd_configure): entry capacity of the pair bins in units of N x S
                       // (3: every resident state a pair, with a margin of three -- a sparse K^n; a K^n of 5..8 latents per
                       // state leaves 10..28 pairs per state: the dense bench asks for 12 = 7.7 GB at the north-star shape)
  int bins_scale_cur = 0;  // what the bins are allocated for right now (ensure_bins_capacity re-cuts them when K^n densifies)
  int bins_auto = 1;       // option "pair_bins_auto": grow the bins from the census of the last statistics pass
  bool bins_dirty = false;  // a binned producer was enqueued and the reduce kernel that zeroes pbins.gcnt was not (a pass
                            // that returned part-way): the next pass clears the region counters before it appends
  int bins_nwg = 2048;  // option "pair_bins_nwg" (read by evoamd_configure): producer workgroups = private regions per bin
  int bsc_wave_opt = 1;  // option "bsc_stats_wave": EBSC statistics on the wave-per-datapoint kernel (0: round-1 kernel)
  int gemm_ws_opt = 1;  // option "gemm_workspace": stream-K partial tiles through a workspace + reduce kernel (0: f64 atomics)
  DevBuf<double> gemm_ws;  // partial tiles of the stream-K contractions (gemm_sk_reduce_kernel adds them to C)
  int pair_bins = 1;
  int gemm_streamk = 1;  // option "gemm_streamk": long-K 128-tile contraction as one resident-sized stream-K grid
  int sk_spare = -1;  // option "sk_spare": workgroups per XCD the FORKED stream-K contraction leaves unlaunched, so that the
                     // H x H elimination chain on the main stream finds free CU slots beside it (a persistent grid of
                     // 2 workgroups per CU otherwise holds every slot until the product is done); -1 = automatic
                     // (StatsPlan::gemm_spare)
  int sssc_prec32 = 0;  // option "sssc_precision" = 32: SSSC(precision=np.float32), see evoamd_set_option in the header
  int main_unstaged = 1;  // option "lpj_main_unstaged": candidate batches on the table-driven lpj kernel without staged B rows
  // option "lpj_singular_screen": exactly singular Psi_A above two latents the reference's way (kernels_sssc.hpp,
  // sssc_exact_mode) -- 0 never, 1 when the tables kernel has stamped this Theta (default), 2 always
  int sing_screen = 1;
  // states above SSSC_KCAP active latents (H > SSSC_KCAP only): slots of global memory for the wavefront kernel's matrices
  DevBuf<double> huge;
  DevBuf<int> huge_ctl;
  int huge_slots = 0, huge_kc = 0;
  int *sing_gen = nullptr;  // view, = err + 4: generation of the last Theta whose Psi held an exactly singular 1x1 / 2x2 block
  int theta_gen = 0;        // stamp of the current Theta (one per sssc_tables_kernel launch)
  int gemm_grouped = 1;  // option "gemm_grouped": grouped split-K instead of stream-K where whole chunks fill the grid
  int gemm_per_xcd = 0;  // option "gemm_per_xcd" (experiments): K chunks per XCD of the 128-tile contraction, 0 = automatic
  evoamd_dense_route route = {};  // what the last dense launcher chose (one host store per call; evoamd_dense_probe returns it)
  double *census = nullptr;  // view: 4 doubles at the head of acc_base, overflow census of the earlier blocks of a chunked statistics pass
  i64 pre_n = 4;
  hipEvent_t ev_chunk[16] = {};
  bool configured = false, have_data = false, have_params = false, have_cand = false, B_valid = false;
  // which ES3C overflow levels (K=4, K=8, LDS) the next pass over K^n needs; exact, from the
  // counters of the last statistics pass (dpar[DP_NGT*]); unknown -> all
  bool need_known = false;
  bool res_need[3] = {true, true, true};
  double res_cnt[3] = {0, 0, 0};  // how many resident states exceeded 2 / 4 / 8 active latents
  bool cand_from_device = false;  // resident candidate batch came from evolve_randflip (k <= k_parent + 1)
  bool lists_clean = false;       // overflow counters are zero (a previous kernel cleared them)
  int pending_skip = 0;           // overflow levels the last lpj chain(s) did not launch: the kernel that clears the
                                  // list counters next checks that their lists stayed empty (err |= 4 otherwise)
  int pays_agreed = -1;           // split all-reduce: -1 not yet agreed over the ranks, else the common decision
  int k8_mode = -1;  // ES3C states with 5..8 active latents: 1 = K=8 register kernel, 0 = LDS wavefront
                     // kernel, -1 = choose per launch from the counts of the last statistics pass
  bool bsc_direct = false;  // EBSC batches: direct residual kernel instead of the Gram-form one
  // EBSC float32 mode (option "ebsc_f32", read by evoamd_configure): the data, B = Y W and the Es rows live in
  // float and the two K- / N-long contractions run on v_mfma_f32_16x16x4_f32; lpj arithmetic, Theta and every
  // accumulator stay double.  Yf (N,D), Ytf = Y^T (D, ldYt), Wf (D,H), Bf (N,H), Esf (N,H)
  bool f32_opt = false, f32 = false;
  DevBuf<float> Yf, Ytf, Wf, Bf, Esf;
  i64 ldYt = 0;
  // double precision: Y^T (D, ldYt) for B = Y W on the 128-tile kernel (large N; option "b_transposed", default 1)
  DevBuf<double> Yt;
  int b_tn_opt = 1;
  DevBuf<uint8_t> mask_infr, mask_x;  // EBSC incomplete data: reliable entries / entries that keep their value
  DevBuf<double> Yrec;  // y_reconstructed (N x D): what the M-step's Wp contraction reads then
  bool yrec_valid = false, rec_in_stats = false;
  DevBuf<double> yhat, tmpWt;  // reconstruction (N x D) and W^T scratch (ES3C)
  bool yhat_valid = false;
  bool keep_differs = false;  // incomplete data: the keep-mask x of evoamd_upload_masks is not x_infr (EBSC sigma, stats_epilogue)
  bool stats_rows_valid = false;  // Es / Ez rows describe the current K^n and Theta
  // evoamd_reconstruct_resident: the selected reconstruction stays on the device for evoamd_patches_merge_resident.
  // rec_resident: y_hat (complete data) / Yrec (incomplete) + the masks below describe it; dropped with yhat_valid and by
  // every upload of data, masks or y_reconstructed.  yrec_from_pass: Yrec was written by the statistics pass y_hat is from.
  bool rec_resident = false, yrec_from_pass = false;
  DevBuf<uint8_t> keep_x;  // complete data: the caller's keep-mask (N x D), uploaded by evoamd_reconstruct_resident
  bool keep_x_valid = false, rec_uses_keep = false;
  DevBuf<uint8_t> row_any;  // incomplete data: datapoint has a reliable entry (N), written by evoamd_upload_masks
  int merge_select_fused = 0;  // option "merge_select_fused" (0: select kernel, then the merge kernels over dense rows -- measured faster)
  // software pipelining across the API boundary: evoamd_mstep_device enqueues the NEXT iteration's pass
  // over the resident K^n behind the mailbox kernel, so the GPU works through the ~40 us the host needs
  // between two iterations; evoamd_lpj_resident then finds it done.  `gen` is bumped by everything that
  // changes what that pass computes (Theta, K^n, data, options).
  unsigned long long gen = 0, prefetch_gen = ~0ull;
  bool prefetch_lpj = true;  // option "prefetch_lpj"
  int spd_block = 0;        // SPD elimination, columns per launch (option "inverse_block"): 0 = 32 from n = 256 on, else 16; 16 / 32 force
  bool use_digest = true;   // lpj / statistics kernels read the state digests (option "state_digest")
  bool spd_inverse = true;  // M-step H x H systems: SPD block Gauss-Jordan first, pivoted path on a bad pivot
  long spd_fallbacks = 0;   // how often the pivoted repeat was needed
  bool rows_fresh = false;  // rowmax / rowsum / Fs partials describe the current lpj (written by vary_kn)
  int model = 0;
  i64 N = 0;
  int D = 0, H = 0, S = 0, S_perm = 0, Cmax = 0, HW = 0, L = 0;
  // data
  DevBuf<double> Y, yy, y2sum;  // SSSC: Y is the left block of [Y | Es | Ez], row stride ldY
  int ldY = 0;
  PinnedBuf<double> h_acc, h_par;  // pinned host staging (accumulator D2H, Theta H2D)
  PinnedBuf<double> h_theta;  // host mailbox (kernels_mstep.hpp: mailbox_kernel): seq | err | tail | dpar | Theta
  double *h_theta_dev = nullptr;  // view: the same memory as the device sees it
  bool h_theta_fresh = false;
  // lazy Theta (evoamd_mstep_device with bit 64): the parameters the E-step ran with, saved on the device before the
  // update overwrites them -- what evoamd_restore_theta_backup re-installs when the update turns out singular
  DevBuf<double> theta_bak;
  bool theta_bak_valid = false;
  unsigned long long mbox_seq = 0;
  DevBuf<unsigned> mbox_counter;
  PinnedBuf<int> h_err;
  // variational state
  DevBuf<u64> states, cand;
  DevBuf<u64> dig, cand_dig;  // state digests (common.hpp), empty when H > DIG_MAX_H
  DevBuf<double> lpj, cand_lpj;
  DevBuf<double> lpj_alt;  // target of the prefetched pass; swapped with lpj when it is consumed (the rows of the
                              // E-step that just ended stay readable until then: sync_to_host, download_lpj)
  DevBuf<int> cand_counts;
  // general device EA (evolve_general_kernel): raw children of a generation, first slot of the last generation,
  // "this known state was duplicated by a child" bits; allocated on first use
  DevBuf<u64> cand_raw, dupold;
  DevBuf<int> gen_start;
  DevBuf<unsigned> flags;  // 3 x N: resident | candidates | permanent
  DevBuf<double> rowmax, rowsum, partial, partial2, diag;  // partial = 3 x partial2.size()
  DevBuf<uint8_t> stage;  // bool staging for (N, max(S,Cmax), H), grown on demand
  // parameters
  DevBuf<double> W, Wt, G, Psi, Bm, mus, pilbar_v;
  DevBuf<double2> GP;
  DevBuf<double4> DG;                // SSSC (H) {mu, pil_bar, G_hh, Psi_hh}
  DevBuf<double4> D1;                // SSSC (H) singleton state terms (sssc_tables_kernel)
  DevBuf<PairEntry> PT;              // SSSC (H,H) pair state terms
  DevBuf<double> pies;               // SSSC (H)
  double *dpar = nullptr;            // view into acc_base: device scalar block (DP_*), kernels read their scalars here
  PinnedBuf<double> h_dpar;          // pinned mirror
  DevBuf<double> colpart;  // per-workgroup partial column sums, grown on demand
  DevBuf<double> gjwork;  // colp | rowp | perm of the multi-launch Gauss-Jordan inverse
  DevBuf<double> tmpA, tmpB, tmpC;  // (H,H) scratch of the device Theta update
  double ljc = 0;
  // statistics
  double *acc = nullptr;  // view into acc_base
  i64 acc_n = 0;
  // ES3C: second-moment contributions of the overflow kernels (states with > 2 active latents), kept
  // apart from the k = 2 sums so that sssc_finish_kernel can rebuild the lower triangle (2 H^2 doubles
  // in front of acc in the same allocation: one memset clears both)
  DevBuf<double> acc_base;
  i64 ovf_n = 0;
  DevBuf<double> Es_own;  // BSC: (N,H)
  double *Es = nullptr;   // view: Es_own (BSC) / columns D..D+H of c->Y (SSSC, Ez follows)
  DevBuf<int> list1, list2, list3, list_n, err;  // list1..3: one size (ensure_lists)
  // ES3C census lists (kernels_sssc_quad.hpp): the resident states with 3..4 / 5..8 / > 8 active latents, built by ONE
  // pass over the digests whenever K^n has changed (kn_gen) and shared by the statistics pass and the next pass over
  // K^n; clist = 3 lists of LIST_SHARDS x list_cap(N S) entries, clist_n = their shard counters (4 x LIST_SHARDS, like
  // list_n); ovf_rec = one record per resident state (only the listed ones are ever touched)
  DevBuf<int> clist, clist_n;
  size_t clist_words() const { return clist.size() / 3; }
  DevBuf<OvfRec> ovf_rec;
  unsigned long long kn_gen = 1, census_gen = 0;
  int census_opt = 1;   // option "census_lists": 0 = round-2 level chains everywhere
  // option "merge_small_levels": with few states above four active latents (census of the last statistics pass) the
  // pivoting wavefront kernel serves the 5..8 list too, instead of a quad launch of its own (3 passes x ~10-20 us)
  int merge_small = 1;
  // ES3C kappa records (kernels_sssc.hpp: sssc_stats_wave_kernel<.., KAP>): {kappa_0, kappa_1} per resident state (N x S) and
  // per candidate (N x Cmax), written by the table-driven lpj kernels beside the lpj, carried by the selection kernel, read by
  // the statistics pass instead of the B rows and the state-term tables.  Allocated by evoamd_configure where the route
  // can run (kappa_shape_ok).  kap_gen / cand_kap_gen: the `gen` they were written (or carried into) -- valid while equal
  // to c->gen; kap_carry: the selection that is being enqueued moves the records with the states.
  DevBuf<double2> kap, cand_kap;
  unsigned long long kap_gen = ~0ull, cand_kap_gen = ~0ull;
  bool kap_carry = false;
  int stats_kappa = 1;  // option "stats_kappa": 0 never / 1 from kappa_min resident states on / 2 wherever the shape allows it
  int kappa_min = 16384;  // option "stats_kappa_min": the automatic setting takes the route from this many resident states
                          // (x 1024) on -- measured: N S = 20 M gains 0.07 ms of 3.9, 10 M is even (0.01 of 2.23, inside
                          // the noise), 2.5 M and 0.64 M lose 0.005-0.01 ms (the record stores, the second finish launch
                          // and the fourth plane cost more than the gathers saved)
  int stats_flat = 0;   // option "stats_flat": census mode, states with <= 2 latents on the thread-per-state kernel instead of
                        // the wave-per-datapoint one.  Measured (c4, steady state): 504-539 vs 584 us for the kernel, but the
                        // quad levels then share 256 bin regions instead of 2048 (107 vs 69 us) and N / 8 shards lose: off
  // fused per-datapoint E-step (kernels_fused.hpp): option "fused_estep" 0 never (default: measured slower than the separate
  // passes at every BASELINE shape) / 1 when K^n is sparse enough / 2 whenever the shape allows it; rowF / rowcnt = per-datapoint free-energy term and counters, defer = datapoints the
  // FAST instantiation left to the FULL one (N items + the counter behind them)
  int fused_opt = 0;
  DevBuf<double> rowF;
  DevBuf<int> rowcnt, defer;
  DevBuf<double> fpart;  // 3 x 1024 chain sums of fused_reduce3_kernel
  DevBuf<unsigned long long> fprof;  // -DFUSED_PROFILE builds
  bool last_estep_fused = false;
  bool reduce_pending = false;  // fused E-step: rowF / rowcnt not yet summed into the scalar block (fused_reduce3_kernel)
  long fused_calls = 0, unfused_calls = 0;
  int debug_poison_list = 0;  // option "debug_poison_list" (tests): the next census gets an out-of-range entry
  int debug_fail_stats = 0;   // option "debug_fail_stats" (tests): the next statistics pass (ES3C, complete data) returns
                              // after its main kernel; any other pass disarms it
  int census_skip = 0;  // levels that passes over the CURRENT census did not launch (checked when it is rebuilt)
  // scratch for single / shared evaluations
  DevBuf<double> tmp_y, tmp_lpj;
  DevBuf<u64> tmp_states;
  // evoamd_loglik_exact: running maximum / sum / marginal sums per datapoint and the outputs (one allocation, grown on demand)
  DevBuf<double> exact_buf;
  // evoamd_patches_*: image and patch rows on the device, grown on demand (never the EM state above)
  DevBuf<double> patch_img, patch_Y;
  DevBuf<double> patch_V;  // evoamd_patches_merge_weighted: the variances of the patch rows
  // evoamd_predictive_moments (kernels_predictive.hpp): mean | var (N x D each), the status word per datapoint and W^T
  // (H x D, transposed from W by every call), grown on demand (never the EM state above); pred_N = 0: nothing to download
  DevBuf<double> pred_buf, pred_Wt;
  DevBuf<int> pred_status;
  i64 pred_N = 0;
  int pred_D = 0;
  // evoamd_predictive_score (kernels_predictive_score.hpp): y_true, then logp | pit (N x D each), logp_n (N), the
  // partials (2 grid) and the total (2); the query bytes (N x D); count | nbad | status (N each); the list of the visited
  // datapoints and their number (N + 1).  Grown on demand, rewritten by every call (W^T goes through pred_Wt)
  DevBuf<double> pscore_y, pscore_d;
  DevBuf<uint8_t> pscore_q;
  DevBuf<int> pscore_i;
  DevBuf<i64> pscore_list;
  // evoamd_posterior_sample (kernels_posterior_sample.hpp): the outputs of the last call and the status word per datapoint,
  // grown on demand and released by evoamd_configure (never the EM state above; W^T goes through pred_Wt, rewritten by
  // every call); ps_keep < 0: nothing to download
  DevBuf<int> ps_slot, ps_status;
  DevBuf<u64> ps_s;
  DevBuf<double> ps_z, ps_y;
  i64 ps_N = 0, ps_T = 0;
  int ps_D = 0, ps_H = 0, ps_keep = -1;
  // evoamd_loglik_estimate (kernels_loglik_estimate.hpp): the running values and outputs per datapoint, log r and t of a
  // pass's outside draws, the clamp flag words of its lpj launches (never those of the EM state) and, with keep_draws, the
  // draws of the last call; grown on demand and released by evoamd_configure; lle_keep < 0: nothing to download
  DevBuf<double> lle_d, lle_keep_d, lle_rho;  // lle_rho: the proposal of every datapoint, kept between the passes of a call
  DevBuf<int> lle_i;
  DevBuf<unsigned> lle_flags;
  DevBuf<u64> lle_keep_s, lle_hash;  // lle_hash: the hashes of K^n's states, kept between the passes of a call
  DevBuf<uint8_t> lle_keep_in;
  i64 lle_N = 0, lle_T = 0;
  int lle_H = 0, lle_keep = -1;
  // evoamd_posterior_codes: the compact outputs on the device (one allocation, grown on demand); rows_kn_gen = the K^n
  // the rows of the last statistics pass were formed from; option "codes_path" (-1 automatic, else CODES_REG / _LDS / _GMEM)
  DevBuf<uint8_t> codes_buf;
  unsigned long long rows_kn_gen = 0;
  int codes_path = -1;
  // evoamd_init_states (kernels_init.hpp): option "init_states_home" (-1 automatic, 0 LDS, 1 global memory), the slots of
  // the global home (grown on demand), and kn_lost: the call stopped at its round cap, K^n is partly written -- every pass
  // that reads K^n refuses until an upload or a successful evoamd_init_states
  int init_home = -1;
  DevBuf<u64> init_scratch;
  DevBuf<double2> seed_gpt;  // evoamd_seed_states, ES3C: the transpose of GP (H x H), grown on demand, rewritten by every call
  DevBuf<double> seed_rows;  // evoamd_seed_states_ex / evoamd_sweep_*_ex, ES3C on incomplete data: the rows of G(n) that do not fit LDS, grown on demand
  // evoamd_refine_states: one row {Fs, new unique, swapped} per iteration; evoamd_posterior_scores: its (N) outputs.  Grown on
  // demand, rewritten by every call, read by nothing else
  DevBuf<double> refine_trace, score_buf;
  // evoamd_sweep_propose / evoamd_sweep_states: the scores of the emitted rows (N, Cmax) and the gains (N); best_flip and
  // n_capped (N each).  Grown on demand.
  DevBuf<double> sweep_d;
  DevBuf<int> sweep_i;
  // evoamd_sweep_*_nb with EVOAMD_SWEEP_SWAP: swap_gain (N); best_swap (N, 2) and n_capped_swap (N).  Grown on demand.
  DevBuf<double> swap_d;
  DevBuf<int> swap_i;
  // evoamd_neighbour_bound: F | M | F+ | best_score (N each); n_states | n_capped | best_parent | best_flip (N each).  Grown on demand.
  DevBuf<double> nbound_d;
  DevBuf<int> nbound_i;
  // evoamd_ais_loglik (kernels_ais.hpp): betas (T + 1) | log w (N, C) | ll | ess | log_w_mean | log_w_min | log_w_max | F_before |
  // F_after (N each); the chains' flips (N, C); the final states (N, C, HW) with the words of s_start (N, HW) behind them;
  // n_flips (N).  Sized before anything is launched, released by evoamd_configure.
  DevBuf<double> ais_d;
  DevBuf<int> ais_i;
  DevBuf<u64> ais_s;
  DevBuf<i64> ais_nf;
  // evoamd_ais_posterior (kernels_ais_post.hpp): p | p_se (N, H each) | mean (N, D; only when asked for) | betas (T + 1) | log w |
  // best lpj | weights (N, C each) | count | map_lpj | ll | ess | log_w_mean | log_w_min | log_w_max (N each); the rows r_c. of
  // one block of datapoints (at most AIS_POST_ROWS_BYTES); the chains' flips (N, C); the chains' best states (N, C, HW) with
  // map_state (N, HW) behind them; n_flips (N).  Sized before anything is launched, released by evoamd_configure.
  // aisp_lds_set: bit log2(NC) = that instantiation has its dynamic LDS limit raised.
  DevBuf<double> aisp_d, aisp_rows;
  DevBuf<int> aisp_i;
  DevBuf<u64> aisp_s;
  DevBuf<i64> aisp_nf;
  unsigned aisp_lds_set = 0;
  unsigned ais_lds_set = 0;  // evoamd_ais_loglik on incomplete data: bit log2(NC) forward, 8 bits up reverse
  // evoamd_remap_latents: K^n in the new latent numbering and its digests, [index (H_new) | n_replaced (N)] and the sum;
  // grown on demand, NOT sized by the geometry: they survive the configure between the remap and
  // evoamd_adopt_remapped_states, which swaps them in and releases them.  remap_H = 0: nothing to adopt.
  // evoamd_latent_map_counts: its (64 HW) counters
  DevBuf<u64> remap_states, remap_dig;
  DevBuf<int> remap_i;
  DevBuf<unsigned long long> remap_sum, map_counts;
  i64 remap_N = 0;
  int remap_S = 0, remap_H = 0;
  // evoamd_resize_states: K^n at the new S, its digests and src_slot (N, S_new); grown on demand and kept through the
  // configure between the resize and evoamd_adopt_resized_states, like the remap scratch.  resize_S = 0: nothing to adopt.
  DevBuf<u64> resize_states, resize_dig;
  DevBuf<int> resize_src;
  i64 resize_N = 0;
  int resize_S = 0, resize_H = 0;
  // the K^n (kn_gen) the rows in lpj were computed for or uploaded beside; selection carries it along (it writes the lpj of
  // every state it swaps in)
  unsigned long long lpj_kn_gen = 0;
  bool kn_lost = false;
  i64 kn_refill = 0;  // while kn_lost: rows [0, kn_refill) have been uploaded again by evoamd_upload_states_packed
  // evoamd_generate (kernels_generate.hpp): Theta^gen, the given states and the outputs of the last call, grown on demand
  // (never the EM state above); gen_keep < 0: no call has completed
  DevBuf<double> gen_par, gen_y, gen_z, gen_ymean;
  DevBuf<u64> gen_sin, gen_s;
  i64 gen_N = 0;
  int gen_D = 0, gen_H = 0, gen_keep = -1;
  // rccl
  void *comm = nullptr;
  int rank = 0, world = 1;
  // timing
  bool timing = false;
  u64 timing_mask = ~0ull;  // which kernel classes record events (each record costs ~5 us of stream time)
  std::vector<TimedSpan> spans;
  std::vector<hipEvent_t> pool;
  double t_ms[KID_COUNT] = {0};
  i64 t_n[KID_COUNT] = {0};
};

// ---- validity: begin
// What is still valid (DESIGN: what a change invalidates).  The flags and generation counters written below are written
// here and nowhere else: a call site says what happened, the function says what that invalidates.  on_*: an input
// changed; made_* / drop_*: a product exists / is gone.  Readers read the fields directly.  (rec_in_stats is also armed
// through the option table, like every option.)
// what hangs on the last statistics pass: y_hat, the [Es | Ez] rows, the resident reconstruction, Yrec as that pass wrote it
static void drop_stats_products(evoamd_ctx *c) { c->yhat_valid = c->stats_rows_valid = c->rec_resident = c->yrec_from_pass = false; }
static void drop_prefetch(evoamd_ctx *c) { c->prefetch_gen = ~0ull; }  // consumed, or no longer what the next pass computes
static void made_prefetch(evoamd_ctx *c) { c->prefetch_gen = c->gen; }
static void drop_B(evoamd_ctx *c) { c->B_valid = false; }  // B = Y W: Theta-derived values are being rebuilt
static void made_B(evoamd_ctx *c) { c->B_valid = true; }
static int next_theta_stamp(evoamd_ctx *c) { return ++c->theta_gen; }  // one per build of the state-term tables

// Nothing the previous configuration left is valid; every generation counter moves on.
static void on_configure(evoamd_ctx *c) {
  c->gen++;
  c->kn_gen++;
  c->census_gen = 0;
  c->pending_skip = c->census_skip = 0;
  c->have_data = c->have_params = c->have_cand = c->rows_fresh = c->acc_clean = c->clist_clean = false;
  c->h_theta_fresh = c->theta_bak_valid = c->yrec_valid = c->rec_in_stats = c->keep_x_valid = c->kn_lost = false;
  c->lists_clean = c->need_known = c->cand_from_device = false;  // fresh (uninitialised) overflow counters
  c->kap_gen = c->cand_kap_gen = ~0ull, c->kap_carry = false;
  // gap: a context that goes from ES3C to EBSC keeps last_estep_fused; if it was set, EBSC never prefetches (only slower)
  if (c->model == EVOAMD_MODEL_SSSC) c->last_estep_fused = false;
  drop_stats_products(c);
  c->pred_N = 0;
  c->rel_frac = -1.0;
  c->pays_agreed = -1;
}
// an option can change which kernel form evaluates K^n: a prefetched pass is dropped
static void on_option(evoamd_ctx *c) { c->gen++; }
static void on_option_changes_derived(evoamd_ctx *c) { c->have_params = false; }  // bsc_direct: G / B are (not) needed, set_params again
// ---- the data
static void on_data_uploaded(evoamd_ctx *c) {
  c->have_data = true;
  c->gen++;
  c->B_valid = false;
  c->rec_resident = false;
  // gap: stats_rows_valid and yhat_valid stand -- evoamd_reconstruct / evoamd_posterior_codes still serve the old data's rows
}
// `present`: masks arrived (Y, yy and hence B changed); else they were removed, which leaves Y as it is
static void on_masks_changed(evoamd_ctx *c, bool present) {
  c->yrec_valid = c->rec_resident = c->yrec_from_pass = false;
  if (present) c->B_valid = false;
  // gap: gen stands -- a pass prefetched on complete data is still consumed by the next evoamd_lpj_resident
}
static void on_yrec_uploaded(evoamd_ctx *c) { c->yrec_valid = true, c->rec_resident = c->yrec_from_pass = false; }
// ---- Theta
static void on_theta_installed(evoamd_ctx *c) {  // by the caller (evoamd_set_params_*), derived values rebuilt
  c->have_params = true;
  c->gen++;
  c->h_theta_fresh = false;
  drop_stats_products(c);
}
static void on_theta_update_begun(evoamd_ctx *c) { c->gen++; }
// Updated on the device.  Unlike an install this keeps y_hat and the resident reconstruction: they were formed under the
// Theta of the E-step on purpose (evoamd_mstep_device bit 32) and are fetched after the update.
static void on_theta_updated(evoamd_ctx *c, bool backup_rode_along) {
  c->B_valid = false;
  if (backup_rode_along) c->theta_bak_valid = true;
  c->stats_rows_valid = false;  // the rows belong to the previous Theta now
}
// The raw parameters of the last E-step are back (the Theta y_hat was formed under: the statistics products stay).
static void on_theta_restored(evoamd_ctx *c) {
  c->gen++;
  c->h_theta_fresh = false;
  c->B_valid = false;
  // gap: G and the state-term tables still belong to the failed update until the next set_params, yet a pass may run
  c->have_params = true;  // evoamd_get_params_* may read them
  drop_prefetch(c);
}
// status 1 / 2: what was derived and prefetched behind the mailbox ran with the failed update's Theta
static void on_theta_update_failed(evoamd_ctx *c) { c->prefetch_gen = ~0ull, c->have_params = false; }
static void made_theta_backup(evoamd_ctx *c) { c->theta_bak_valid = true; }
static void drop_theta_backup(evoamd_ctx *c) { c->theta_bak_valid = false; }
static void made_theta_mailbox(evoamd_ctx *c, bool holds_theta) { c->h_theta_fresh = holds_theta; }
// ---- K^n
// K^n changed: the prefetched pass, the census and the rows of the last statistics pass describe the old one.  Selection
// keeps the level hints (the counts of the last statistics pass remain the best estimate); a K^n from the caller drops them.
enum KnBy { KN_BY_CALLER, KN_BY_SELECTION };
static void on_kn_changed(evoamd_ctx *c, KnBy by) {
  // the kappa records follow K^n through a selection only, and only when both sides hold current ones (made_selection
  // stamps them again); every other event -- and every other gen++ above and below -- leaves them behind
  c->kap_carry = by == KN_BY_SELECTION && c->kap_gen == c->gen && c->cand_kap_gen == c->gen;
  const bool rows_follow = by == KN_BY_SELECTION && c->lpj_kn_gen == c->kn_gen;
  c->gen++;
  c->kn_gen++;
  if (rows_follow) c->lpj_kn_gen = c->kn_gen;
  if (by == KN_BY_CALLER) c->need_known = false;
}
// kappa records (ES3C, option "stats_kappa"): the pass over K^n / over the candidate batch wrote them under this gen (or not)
static void made_kappa(evoamd_ctx *c, bool written) { c->kap_gen = written ? c->gen : ~0ull; }
static void made_cand_kappa(evoamd_ctx *c, bool written) { c->cand_kap_gen = written ? c->gen : ~0ull; }
static void on_kn_complete(evoamd_ctx *c) { c->kn_lost = false; }  // a whole K^n arrived: upload, or evoamd_init_states to its end
// evoamd_init_states begun: K^n counts as lost until the kernel has completed every datapoint (stopped at its round cap:
// no event, it stays lost)
static void on_kn_init_begun(evoamd_ctx *c) {
  c->kn_lost = true, c->kn_refill = 0;
  on_kn_changed(c, KN_BY_CALLER);
}
// rows [n0, n0 + n) replaced: not a whole K^n, but chunks in ascending order rebuild a lost one
static void on_kn_rows_uploaded(evoamd_ctx *c, i64 n0, i64 n) {
  on_kn_changed(c, KN_BY_CALLER);
  if (c->kn_lost && n0 <= c->kn_refill && n0 + n > c->kn_refill) {
    c->kn_refill = n0 + n;
    if (c->kn_refill >= c->N) c->kn_lost = false;
  }
}
static void on_estep_route(evoamd_ctx *c, bool fused) { c->last_estep_fused = fused; }  // (a fused E-step evaluates K^n itself: no prefetch)
// ---- lpj rows, row statistics, counters a kernel clears on its way
static void on_lpj_overwritten(evoamd_ctx *c) { c->rows_fresh = false; }  // rowmax / rowsum / Fs partials describe other rows
static void made_row_stats(evoamd_ctx *c) { c->rows_fresh = true; }
static void made_lpj_rows(evoamd_ctx *c) { c->lpj_kn_gen = c->kn_gen; }  // the rows in lpj are those of the resident K^n
// a chain is about to append to the on-the-fly lists; the caller has checked + cleared them unless they were clean
static void on_lists_claimed(evoamd_ctx *c) {
  if (!c->lists_clean) c->pending_skip = 0;
  c->lists_clean = false;
}
// a kernel zeroed the overflow counters and checked the skipped levels of the chain before it (ES3C has such lists)
static void made_clean_lists(evoamd_ctx *c) {
  c->lists_clean = c->model == EVOAMD_MODEL_SSSC;
  if (c->lists_clean) c->pending_skip = 0;
}
// the levels a pass did not launch (launch_sssc_lpj has the table): whoever clears the counters next checks them
static void on_levels_skipped(evoamd_ctx *c, bool census_route, int skipped, int served, bool any) {
  if (census_route) {
    c->census_skip |= skipped;
    if (any && !(served & 2)) c->pending_skip |= 2;
  } else {
    c->pending_skip = (c->pending_skip | skipped) & ~served;
  }
}
// the selection kernel: row statistics of the new lpj rows, and on its way the old census checked + cleared, the
// accumulators of the next statistics pass zeroed, the on-the-fly lists cleared
static void made_selection(evoamd_ctx *c, bool census_cleared, bool acc_zeroed, bool kappa_carried) {
  made_row_stats(c);
  if (kappa_carried && c->kap_carry) c->kap_gen = c->gen;
  c->kap_carry = false;
  if (census_cleared) {
    c->clist_clean = true;
    c->census_skip = 0;
  }
  c->acc_clean = acc_zeroed;
  made_clean_lists(c);
}
// ---- census
// its counters were checked; a kernel is about to append to the lists
static void on_census_claimed(evoamd_ctx *c) { c->clist_clean = false, c->census_skip = 0; }
static void made_census(evoamd_ctx *c) { c->census_gen = c->kn_gen; }
static void on_census_poisoned(evoamd_ctx *c) { c->kn_gen++; }  // test hook: rebuilt before anything else reads it
// ---- candidates
// `near_parents`: children of evolve_randflip (k <= k_parent + 1: the overflow levels take a shortcut); a batch from the
// host or from the general operators may differ from every resident state in many bits
static void on_cand_installed(evoamd_ctx *c, bool near_parents) { c->cand_from_device = near_parents, c->cand_kap_gen = ~0ull; }
static void made_cand_lpj(evoamd_ctx *c) { c->have_cand = true; }
// the candidate buffers were borrowed for states that are no children of K^n (the importance draws of
// evoamd_loglik_estimate): no batch counts as installed, evoamd_vary_kn refuses until the next one
static void drop_cand_batch(evoamd_ctx *c) { c->have_cand = false, c->cand_from_device = false, c->cand_kap_gen = ~0ull; }
// fused E-step: K^n advanced, its rows and (small shards) its census came with it, the children never left the kernel
static void made_fused_estep(evoamd_ctx *c, bool inkernel_census) {
  on_kn_changed(c, KN_BY_SELECTION);
  if (inkernel_census) made_census(c);
  made_row_stats(c);
  made_lpj_rows(c);  // (the fused kernel evaluates K^n itself and keeps the rows of what it swaps in)
  c->kap_carry = false;  // the fused kernel carries no kappa records
  c->have_cand = false, c->cand_from_device = true;
  on_estep_route(c, true);
}
static void made_fused_rows(evoamd_ctx *c, bool reduced) { c->reduce_pending = !reduced; }  // rowF / rowcnt written / summed into the scalar block
// ---- statistics pass and what is made of it
static void on_bins_append(evoamd_ctx *c) { c->bins_dirty = true; }  // until the reduce kernel that zeroes the region counters
static void made_bins_clean(evoamd_ctx *c) { c->bins_dirty = false; }
static void on_stats_pass_begun(evoamd_ctx *c) {  // accumulators zeroed, region counters clean; the last pass's products go
  c->bins_dirty = false;
  c->acc_clean = false;
  drop_stats_products(c);
}
static void made_stats_rows(evoamd_ctx *c) { c->stats_rows_valid = true, c->rows_kn_gen = c->kn_gen; }
// After the accumulator + scalar block reached the host: remember which overflow levels K^n needs.
static void made_level_hints(evoamd_ctx *c, const double *dpar_host) {
  if (c->model != EVOAMD_MODEL_SSSC) return;
  for (int j = 0; j < 3; j++) {
    c->res_cnt[j] = dpar_host[DP_NGT2 + j];
    c->res_need[j] = c->res_cnt[j] > 0.0;
  }
  c->need_known = true;
}
static void made_wq_copy(evoamd_ctx *c, bool present) { c->wq_copy_valid = present; }  // EBSC: tmpA holds Wq (false: inverted in place)
static void made_yhat(evoamd_ctx *c) { c->yhat_valid = true; }
// Yrec selected from the y_hat of this pass; `in_stats`: by the pass itself, which serves the one-shot option
static void made_yrec_from_pass(evoamd_ctx *c, bool in_stats) {
  c->yrec_valid = c->yrec_from_pass = true;
  if (in_stats) c->rec_in_stats = false;
}
static void drop_resident_rec(evoamd_ctx *c) { c->rec_resident = false; }
static void on_keep_mask(evoamd_ctx *c, bool uploaded) { c->keep_x_valid = uploaded; }
static void made_resident_rec(evoamd_ctx *c, bool uses_keep) { c->rec_uses_keep = uses_keep, c->rec_resident = true; }
static void made_predictive(evoamd_ctx *c, i64 N) { c->pred_N = N; }  // 0: nothing to download
static void made_generated(evoamd_ctx *c, int keep) { c->gen_keep = keep; }  // -1: no call has completed
static void made_posterior_samples(evoamd_ctx *c, int keep) { c->ps_keep = keep; }  // -1: nothing to download (no EM state reads it)
static void made_remap(evoamd_ctx *c, i64 N, int S, int H_new) { c->remap_N = N, c->remap_S = S, c->remap_H = H_new; }  // 0: nothing to adopt
static void made_resize(evoamd_ctx *c, i64 N, int S_new, int H) { c->resize_N = N, c->resize_S = S_new, c->resize_H = H; }  // 0: nothing to adopt
static void made_loglik_draws(evoamd_ctx *c, int keep) { c->lle_keep = keep; }  // -1: nothing to download (no EM state reads it)
// ---- validity: end

struct SpanGuard {
  evoamd_ctx *c;
  int kid;
  hipStream_t stream;  // where the span's work is enqueued: the main stream unless the caller names another
  hipEvent_t a = nullptr, b = nullptr;
  SpanGuard(evoamd_ctx *ctx, int k, hipStream_t s = nullptr) : c(ctx), kid(k), stream(s ? s : ctx->stream) {
    if (!c->timing || !((c->timing_mask >> k) & 1ull)) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!c->pool.empty()) {
        e = c->pool.back();
        c->pool.pop_back();
      } else {
        (void)hipEventCreate(&e);
      }
      return e;
    };
    a = get();
    b = get();
    (void)hipEventRecord(a, stream);
  }
  ~SpanGuard() {
    if (!c->timing || !a) return;
    (void)hipEventRecord(b, stream);
    c->spans.push_back({a, b, kid});
  }
};

static int resolve_spans(evoamd_ctx *c) {
  for (auto &s : c->spans) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(s.b));
    HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
    c->t_ms[s.kid] += ms;
    c->t_n[s.kid] += 1;
    c->pool.push_back(s.a);
    c->pool.push_back(s.b);
  }
  c->spans.clear();
  return 0;
}

static inline unsigned cdiv(i64 a, i64 b) { return (unsigned)((a + b - 1) / b); }
// entries one shard of an overflow list can receive from `total` pairs (workgroup batches of 256..1024
// pairs are dealt round-robin to the shards)
static inline size_t list_cap(i64 total) { return (size_t)(256 * (((total + 255) / 256 + LIST_SHARDS - 1) / LIST_SHARDS) + 1024); }

// out[c] += sum_r X[r][c] (out must be zeroed by the caller); SQUARE sums squares.
template <bool SQUARE>
static void launch_colsum(evoamd_ctx *c, const double *X, int ldx, i64 R, int Cn, double *out) {
  const i64 rpb = 256;
  c->route = {EVOAMD_ROUTE_COLSUM, 64, (int)cdiv(R, rpb), 0, 0, 0, 0, 0};
  dim3 grid(cdiv(Cn, 64), cdiv(R, rpb));
  colsum_f64<SQUARE><<<grid, 256, 0, c->stream>>>(X, ldx, R, Cn, rpb, out);
}


// overflow lists big enough for a batch of `total` (datapoint, state) pairs
static int ensure_lists(evoamd_ctx *c, i64 total) {
  const size_t need = list_cap(total) * LIST_SHARDS;
  TRY(c->list1.ensure(c, need));
  TRY(c->list2.ensure(c, need));
  return c->list3.ensure(c, need);
}

// ---------------------------------------------------------------------------------------
// library / context
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_abi_version(void) { return EVOAMD_ABI_VERSION; }
extern "C" const char *evoamd_last_error(void) { return g_err; }

extern "C" int evoamd_device_count(int *count) {
  REQUIRE(count, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(EVOAMD_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return 0;
}

static int kn_set_lds_limits();  // the seeding and sweep kernels: one table, beside their launch plan
// kernels whose dynamic LDS exceeds the 64 KiB a launch may ask for by default
static int set_kernel_lds_limits() {
  HIP_TRY(hipFuncSetAttribute((const void *)sssc_stats_flat_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)sssc_big_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              136 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)sssc_big_kernel<0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              136 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)sssc_big_kernel<0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              136 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)sssc_big_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              136 * 1024));
  HIP_TRY(hipFuncSetAttribute((const void *)posterior_codes_kernel<CODES_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              CODES_WAVES * CODES_LDS_H * (int)sizeof(double)));
  HIP_TRY(hipFuncSetAttribute((const void *)gemm_tn128_f64, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)GEMM128_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute((const void *)gemm_tn128_rows_f64, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)GEMM128_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute((const void *)gemm_tn128_sk_f64, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)GEMM128_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute((const void *)gemm_tn128_sk_f32, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)GEMM128_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute((const void *)gemm_tn128_store_f32, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)GEMM128_LDS_BYTES));
  {
    const int lds = (int)(PRED_WAVES * pred_lds_doubles(PRED_MAX_K, true) * sizeof(double));
    const void *pk[] = {(const void *)predictive_kernel<1, true>, (const void *)predictive_kernel<2, true>,
                        (const void *)predictive_kernel<4, true>, (const void *)predictive_kernel<8, true>};
    for (const void *f : pk) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const void *sk[] = {(const void *)posterior_sample_kernel<1, true>, (const void *)posterior_sample_kernel<2, true>,
                        (const void *)posterior_sample_kernel<4, true>, (const void *)posterior_sample_kernel<8, true>};
    for (const void *f : sk) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const void *ck[] = {(const void *)predictive_score_kernel<1, true>, (const void *)predictive_score_kernel<2, true>,
                        (const void *)predictive_score_kernel<4, true>, (const void *)predictive_score_kernel<8, true>};
    for (const void *f : ck) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  HIP_TRY(hipFuncSetAttribute((const void *)remap_latents_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, REMAP_LDS_BYTES));
  HIP_TRY(hipFuncSetAttribute((const void *)resize_states_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RESIZE_LDS_BYTES));
  TRY(kn_set_lds_limits());
  {
    const void *wk[] = {(const void *)sssc_stats_wave_kernel<0, 4>,  (const void *)sssc_stats_wave_kernel<1, 4>,
                        (const void *)sssc_stats_wave_kernel<2, 4>,  (const void *)sssc_stats_wave_kernel<4, 4>,
                        (const void *)sssc_stats_wave_kernel<8, 4>,  (const void *)sssc_stats_wave_kernel<16, 4>,
                        (const void *)sssc_stats_wave_kernel<0, 1>,  (const void *)sssc_stats_wave_kernel<0, 8>,
                        (const void *)sssc_stats_wave_kernel<0, 16>, (const void *)sssc_stats_wave_kernel<1, 4, true, true>};
    for (const void *f : wk) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));  // + <= 9.2 KiB static
    HIP_TRY(hipFuncSetAttribute((const void *)pair_bins_reduce_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * PB_TILE * 8));
    HIP_TRY(hipFuncSetAttribute((const void *)pair_bins_reduce_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * PB_TILE * 8));
    HIP_TRY(hipFuncSetAttribute((const void *)sssc_small_kernel<4, 1, 2, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024));
    HIP_TRY(hipFuncSetAttribute((const void *)sssc_small_kernel<8, 1, 2, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024));
  }
  {
    const void *fk[] = {(const void *)sssc_estep_fused_kernel<1, false>,  (const void *)sssc_estep_fused_kernel<1, true>,
                        (const void *)sssc_estep_fused_kernel<2, false>,  (const void *)sssc_estep_fused_kernel<2, true>,
                        (const void *)sssc_estep_fused_kernel<4, false>,  (const void *)sssc_estep_fused_kernel<4, true>,
                        (const void *)sssc_estep_fused_kernel<8, false>,  (const void *)sssc_estep_fused_kernel<8, true>,
                        (const void *)sssc_estep_fused_kernel<16, false>, (const void *)sssc_estep_fused_kernel<16, true>};
    for (const void *fp : fk) HIP_TRY(hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  return 0;
}

extern "C" int evoamd_ctx_create(int device, evoamd_ctx **out) {
  REQUIRE(out, "out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(EVOAMD_E_NODEVICE, "no HIP device visible (libevo_amd needs an MI355X / gfx950 GPU)");
  REQUIRE(device >= 0 && device < n, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EVOAMD_E_NODEVICE, "device %d is %s; libevo_amd is built for gfx950 only", device,
                prop.gcnArchName);
  std::unique_ptr<evoamd_ctx> guard(new evoamd_ctx());  // every early return destroys what was created so far
  evoamd_ctx *c = guard.get();
  c->device = device;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    // the main stream carries the latency-bound chains (Theta update, small launches), stream2 the forked MFMA
    // contraction: the dispatcher serves the higher priority first whenever a CU slot is free
    int prio_lo = 0, prio_hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    HIP_TRY(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi));
    HIP_TRY(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_lo));
  }
  HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_theta, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_theta_done, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_mbox, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_bak, hipEventDisableTiming));
  for (int i = 0; i < 16; i++) HIP_TRY(hipEventCreateWithFlags(&c->ev_chunk[i], hipEventDisableTiming));
  TRY(set_kernel_lds_limits());
  *out = guard.release();
  return 0;
}

static int sync_streams(evoamd_ctx *c) {
  for (hipStream_t s : {c->stream, c->stream2, c->stream_copy})
    if (s) HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

evoamd_ctx::~evoamd_ctx() {
  (void)hipSetDevice(device);
  (void)sync_streams(this);  // nothing in flight reads a buffer or records an event once the members go
  if (comm && g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
  for (auto &s : spans) {
    (void)hipEventDestroy(s.a);
    (void)hipEventDestroy(s.b);
  }
  for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  for (hipStream_t s : {stream, stream2, stream_copy})
    if (s) (void)hipStreamDestroy(s);
  for (hipEvent_t e : {ev_fork, ev_join, ev_theta, ev_theta_done, ev_mbox, ev_bak})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_chunk)
    if (e) (void)hipEventDestroy(e);
}

extern "C" void evoamd_ctx_destroy(evoamd_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

extern "C" int evoamd_debug_live_buffers(int64_t out[2]) {
  REQUIRE(out, "out is NULL");
  out[0] = g_live_dev;
  out[1] = g_live_pinned;
  return 0;
}

extern "C" int evoamd_debug_validity(evoamd_ctx *c, int64_t out[8]) {
  REQUIRE(c && out, "ctx / out is NULL");
  const bool bits[32] = {c->have_data,      c->have_params,       c->have_cand,      c->B_valid,
                         c->rows_fresh,     c->stats_rows_valid,  c->yhat_valid,     c->rec_resident,
                         c->yrec_valid,     c->yrec_from_pass,    c->rec_in_stats,   c->keep_x_valid,
                         c->rec_uses_keep,  c->need_known,        c->res_need[0],    c->res_need[1],
                         c->res_need[2],    c->cand_from_device,  c->lists_clean,    c->clist_clean,
                         c->acc_clean,      c->wq_copy_valid,     c->h_theta_fresh,  c->theta_bak_valid,
                         c->kn_lost,        c->last_estep_fused,  c->reduce_pending, c->bins_dirty,
                         c->gen_keep >= 0,  c->prefetch_gen == c->gen, c->census_gen == c->kn_gen, c->rows_kn_gen == c->kn_gen};
  out[0] = 0;
  for (int i = 0; i < 32; i++) out[0] |= (int64_t)bits[i] << i;
  out[1] = (int64_t)c->gen;
  out[2] = (int64_t)c->kn_gen;
  out[3] = c->theta_gen;
  out[4] = c->pending_skip;
  out[5] = c->census_skip;
  out[6] = c->kn_refill;
  out[7] = c->pred_N;
  return 0;
}

// One row per option of evoamd_set_option (what each one means: the comments at the fields of evoamd_ctx).
struct OptionRow {
  const char *name;
  int evoamd_ctx::*ifield;   // where the value goes: an int field ...
  bool evoamd_ctx::*bfield;  // ... or a bool field
  int (*norm)(int) = nullptr;  // how the value is stored (nullptr: as it is)
  int lo = 0, hi = 0;             // with `err`: the accepted range ...
  bool (*accepts)(int) = nullptr;  // ... or set
  const char *err = nullptr;     // the refusal (nullptr: every value is accepted)
  void (*after)(evoamd_ctx *) = nullptr;  // side effect of a successful set
};
#define OPT_INT(f) &evoamd_ctx::f, nullptr
#define OPT_BOOL(f) nullptr, &evoamd_ctx::f
static int opt_flag(int v) { return v != 0; }
static const OptionRow OPTIONS[] = {
    {"sssc_k8", OPT_INT(k8_mode), [](int v) { return v < 0 ? -1 : (int)(v != 0); }},
    {"ebsc_f32", OPT_BOOL(f32_opt), opt_flag},  // takes effect at the next evoamd_configure
    {"bsc_direct", OPT_BOOL(bsc_direct), opt_flag, 0, 0, nullptr, nullptr,
     on_option_changes_derived},
    {"reconstruct_in_stats", OPT_BOOL(rec_in_stats), opt_flag},  // one-shot: the next statistics pass forms y_reconstructed first
    {"codes_path", OPT_INT(codes_path), nullptr, -1, CODES_GMEM, nullptr, "codes_path: -1 (auto), 0 registers, 1 LDS, 2 global memory"},
    {"merge_select_fused", OPT_INT(merge_select_fused), opt_flag},
    {"prefetch_lpj", OPT_BOOL(prefetch_lpj), opt_flag},
    {"inverse_block", OPT_INT(spd_block), nullptr, 0, 0, [](int v) { return v == 0 || v == 16 || v == 32; },
     "inverse_block: 0 (auto), 16 or 32"},
    {"overlap_gemm", OPT_INT(overlap_gemm)},
    {"stats_stage", OPT_INT(stats_stage)},
    {"stats_waves", OPT_INT(stats_waves)},
    {"pair_bins", OPT_INT(pair_bins)},
    {"gemm_streamk", OPT_INT(gemm_streamk)},
    {"b_transposed", OPT_INT(b_tn_opt)},  // takes effect at the next evoamd_configure
    {"pair_bins_scale", OPT_INT(bins_scale), nullptr, 1, 64, nullptr, "pair_bins_scale: 1 .. 64"},
    {"pair_bins_nwg", OPT_INT(bins_nwg), nullptr, 0, 0, [](int v) { return v >= 256 && v <= 2048 && (v % 256) == 0; },
     "pair_bins_nwg: 256 .. 2048, multiple of 256"},
    {"pair_bins_auto", OPT_INT(bins_auto), opt_flag},
    {"pair_bins_min", OPT_INT(bins_min)},
    {"bsc_stats_wave", OPT_INT(bsc_wave_opt)},
    {"gemm_workspace", OPT_INT(gemm_ws_opt)},
    {"sssc_precision", OPT_INT(sssc_prec32), [](int v) { return (int)(v == 32); }, 0, 0, [](int v) { return v == 64 || v == 32; },
     "sssc_precision: 64 or 32"},
    {"lpj_main_unstaged", OPT_INT(main_unstaged), opt_flag},
    {"lpj_singular_screen", OPT_INT(sing_screen), nullptr, 0, 2, nullptr, "lpj_singular_screen: 0 (never), 1 (automatic) or 2 (always)"},
    {"gemm_grouped", OPT_INT(gemm_grouped), opt_flag},
    {"gemm_per_xcd", OPT_INT(gemm_per_xcd)},
    {"init_states_home", OPT_INT(init_home), nullptr, -1, 1, nullptr, "init_states_home: -1 (auto), 0 LDS, 1 global memory"},
    {"background_unit", OPT_INT(bg_unit), opt_flag},
    {"fold_clear", OPT_INT(fold_clear), opt_flag},
    {"early_fork", OPT_INT(early_fork)},
    {"merge_small_levels", OPT_INT(merge_small), opt_flag},
    {"stats_flat", OPT_INT(stats_flat), opt_flag},
    {"theta_copy_engine", OPT_INT(theta_copy_engine), opt_flag},
    {"census_lists", OPT_INT(census_opt), opt_flag},  // takes effect at the next evoamd_configure
    {"sk_spare", OPT_INT(sk_spare), nullptr, -1, 32, nullptr, "sk_spare: -1 (automatic) or 0 .. 32 workgroups per XCD"},
    {"stats_chunks", OPT_INT(stats_chunks), nullptr, 1, 16, nullptr, "stats_chunks: 1 .. 16"},
    {"mailbox_side_stream", OPT_INT(mbox_side), opt_flag},
    {"fused_estep", OPT_INT(fused_opt), nullptr, 0, 2, nullptr, "fused_estep: 0 (never), 1 (automatic) or 2 (whenever the shape allows it)"},
    {"debug_poison_list", OPT_INT(debug_poison_list), opt_flag},
    {"debug_fail_stats", OPT_INT(debug_fail_stats), opt_flag},
    {"state_digest", OPT_BOOL(use_digest), opt_flag},
    {"inverse_spd", OPT_BOOL(spd_inverse), opt_flag},
};
// Options added after tests/test_host_logic.py wrote out the names of the table above (which therefore stays as it is,
// like _lib.KERNEL_IDS); tests/test_stats_kappa_algebra.py holds these to the same rule: documented in include/evo_amd.h
// and listed in INTEGRATION.md.
static const OptionRow OPTIONS_LATER[] = {
  {"stats_kappa", OPT_INT(stats_kappa), nullptr, 0, 2, nullptr, "stats_kappa: 0 (never), 1 (automatic) or 2 (wherever the shape allows it)"},
  {"stats_kappa_min", OPT_INT(kappa_min), nullptr, 0, 1 << 20, nullptr, "stats_kappa_min: 0 .. 1048576 (x 1024 resident states)"},
};
#undef OPT_INT
#undef OPT_BOOL

extern "C" int evoamd_set_option(evoamd_ctx *c, const char *name, int value) {
  REQUIRE(c && name, "bad arguments");
  on_option(c);
  std::vector<const OptionRow *> rows;
  for (const OptionRow &o : OPTIONS) rows.push_back(&o);
  for (const OptionRow &o : OPTIONS_LATER) rows.push_back(&o);
  for (const OptionRow *row : rows) {
    const OptionRow &o = *row;
    if (strcmp(name, o.name) != 0) continue;
    if (o.err && !(o.accepts ? o.accepts(value) : (value >= o.lo && value <= o.hi))) return fail(EVOAMD_E_INVALID, "%s", o.err);
    const int v = o.norm ? o.norm(value) : value;
    if (o.ifield) c->*o.ifield = v;
    else c->*o.bfield = v != 0;
    if (o.after) o.after(c);
    return 0;
  }
  return fail(EVOAMD_E_INVALID, "unknown option '%s'", name);
}

static int join_fork(evoamd_ctx *c);

extern "C" int evoamd_synchronize(evoamd_ctx *c) {
  REQUIRE(c, "ctx is NULL");
  TRY(join_fork(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------
static i64 acc_len(const evoamd_ctx *c) {
  const i64 H = c->H, D = c->D;
  return (c->model == EVOAMD_MODEL_BSC) ? H * D + H * H + H + 1 + 8 : 2 * H + 4 * H * H + D * H + D + 8;
}
// offsets into the packed accumulator
struct AccLayout {
  i64 Wp, Wq, pies, sigma;                                              // BSC
  i64 xs, xss, xsz, xszsz, s_sz, sz_sz, sWp, y2;                        // SSSC
  i64 tail;
};
static AccLayout acc_layout(const evoamd_ctx *c) {
  AccLayout a = {};
  const i64 H = c->H, D = c->D;
  if (c->model == EVOAMD_MODEL_BSC) {
    a.Wp = 0;
    a.Wq = H * D;
    a.pies = a.Wq + H * H;
    a.sigma = a.pies + H;
    a.tail = a.sigma + 1;
  } else {
    a.xs = 0;
    a.xss = H;
    a.xsz = a.xss + H * H;
    a.xszsz = a.xsz + H;
    a.sWp = a.xszsz + H * H;  // Wp | s_sz_outer | sz_sz_outer are one (D+2H) x H GEMM output
    a.s_sz = a.sWp + D * H;
    a.sz_sz = a.s_sz + H * H;
    a.y2 = a.sz_sz + H * H;
    a.tail = a.y2 + D;
  }
  return a;
}

// Pair bins of the statistics pass (pair_bins.hpp): 2 rf folded rows x H columns per LDS tile; `scale` = entry capacity in
// units of N x S 32-byte entries.  An optimisation, not a requirement: if the regions do not fit beside the rest, the
// statistics kernels use their global-atomic paths.
static int alloc_pair_bins(evoamd_ctx *c, int scale) {
  const i64 N = c->N;
  const int H = c->H, S = c->S;
  c->pb_ent.reset();
  c->pb_gcnt.reset();
  c->pb_part.reset();
  c->pbins = PairBins{};
  c->bins_scale_cur = 0;
  if (H >= 2 && H <= 1024) {
    PairBins pb = {};
    pb.rf = std::max(1, PB_TILE / (2 * H));
    const int nfold = (H - 1 + 1) / 2;
    pb.nb = (int)cdiv(nfold, pb.rf);
    // producer workgroups: a resident-sized grid (8 per CU); every one owns a region per bin, sized for all
    // of its states being pairs spread evenly over the bins x 3 (the overflow kernels append behind the main one)
    pb.nwg = c->bins_nwg;
    // reduce workgroups per bin: 4 (8 from 8 M resident states on), and enough of them that bins x workgroups fill
    // the chip -- H = 128 has 4 bins, H = 256 has 16: with 4 workgroups each the reduce ran on 16 / 64 of 256 CUs
    pb.nsh = std::max((i64)N * S >= (i64)8 << 20 ? 8 : 4, std::min(PB_NSH_MAX, 256 / std::max(1, pb.nb)));
    pb.cap = (int)std::max<i64>(64, (i64)scale * cdiv((i64)N * S, (i64)pb.nb * pb.nwg));
    pb.planes = 3;  // (room for four: the ES3C kappa route reduces its passes into four, stats_sssc_block)
    const size_t ne = (size_t)pb.nb * pb.nwg * pb.cap;
    if (c->pb_ent.try_alloc(ne) && c->pb_part.try_alloc((size_t)pb.nb * pb.nsh * (c->model == EVOAMD_MODEL_SSSC ? 4 : 3) * 2 * pb.rf * H) &&
        c->pb_gcnt.try_alloc((size_t)pb.nb * pb.nwg)) {
      pb.ent = c->pb_ent;
      pb.part = c->pb_part;
      pb.gcnt = c->pb_gcnt;
      HIP_TRY(hipMemsetAsync(pb.gcnt, 0, c->pb_gcnt.size() * sizeof(int), c->stream));
      c->pbins = pb;
      c->bins_scale_cur = scale;
      made_bins_clean(c);
    } else {
      c->pb_ent.reset();
      c->pb_part.reset();
      c->pb_gcnt.reset();
    }
  }
  return 0;
}

// The bins were sized at configure time for a sparse K^n (every state a pair, x 3).  A state with k active latents leaves
// k (k - 1) / 2 entries; once the census of the last statistics pass (dpar[DP_NGT*], on the host since the last mailbox)
// says the K^n has outgrown the regions, they are re-cut BEFORE the next pass instead of letting it fall onto the atomic
// fallback (a silent performance cliff: the dense-state variant needed pair_bins_scale = 12 set by hand).  Grows only.
static int ensure_bins_capacity(evoamd_ctx *c) {
  if (c->model != EVOAMD_MODEL_SSSC || !c->need_known || !c->pbins.ent || c->bins_auto == 0) return 0;
  const double NS = (double)c->N * c->S;
  const double n34 = c->res_cnt[0] - c->res_cnt[1], n58 = c->res_cnt[1] - c->res_cnt[2];
  // (3..4 latents: up to 6 pairs, 5..8: up to 28; the states above eight go through the wavefront kernel's atomics)
  const double entries = (NS - c->res_cnt[0]) + 6.0 * n34 + 28.0 * n58;
  int want = (int)std::ceil(3.0 * 1.25 * entries / NS);  // margin 3 like the default, 25 % head room for the next iterations
  if (want > 64) want = 64;
  if (want <= c->bins_scale_cur) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
  const int before = c->bins_scale_cur;
  TRY(alloc_pair_bins(c, want));
  if (!c->pbins.ent) {  // does not fit: back to what there was (or the atomics if even that is gone now)
    TRY(alloc_pair_bins(c, before));
    c->bins_auto = 0;
  }
  return 0;
}

// ES3C kappa route: does the option ask for it at this size?  (Read by evoamd_configure for the record buffers and by
// kappa_shape_ok for every pass.)
static bool kappa_wanted(const evoamd_ctx *c) {
  return c->stats_kappa == 2 || (c->stats_kappa == 1 && c->N * (i64)c->S >= (i64)c->kappa_min * 1024);
}

// ---- evoamd_configure: unconfigured -> validate -> geometry -> drop -> allocate by group -> clear -> flags -> configured ----
static int configure_validate(const evoamd_ctx *c, int model, i64 N, int D, int H, int S, int S_perm, int Cmax) {
  REQUIRE(model == EVOAMD_MODEL_BSC || model == EVOAMD_MODEL_SSSC, "unknown model");
  REQUIRE(N > 0 && D > 0 && H > 0 && S > 0, "N, D, H, S must be positive");
  REQUIRE(S_perm == 0 || S_perm == 1, "S_perm must be 0 or 1");
  REQUIRE(Cmax >= 1 && Cmax <= 64 * VK_MAX_C_PER_LANE, "Cmax must be in [1, 256]");
  REQUIRE(S <= 64 * VK_MAX_S_PER_LANE, "S must be <= 1024");
  REQUIRE((i64)N * (S > Cmax ? S : Cmax) < 2147483647LL, "N * max(S, Cmax) must fit in int32");
  if (model == EVOAMD_MODEL_BSC && c->f32_opt)
    REQUIRE((H % 4) == 0 && (D % 4) == 0, "float32 mode needs H and D to be multiples of 4 (16-byte rows)");
  return 0;
}

static void configure_geometry(evoamd_ctx *c, int model, i64 N, int D, int H, int S, int S_perm, int Cmax) {
  c->model = model;
  c->N = N;
  c->D = D;
  c->H = H;
  c->S = S;
  c->S_perm = S_perm;
  c->Cmax = Cmax;
  c->HW = (H + 63) / 64;
  c->L = S + S_perm;
  c->ldY = (model == EVOAMD_MODEL_SSSC) ? D + 3 * H : D;  // ES3C: [Y | Es | Ez | Ed]
  c->f32 = model == EVOAMD_MODEL_BSC && c->f32_opt;
  c->acc_n = acc_len(c);
  // in front of the packed accumulator, cleared by the same memset: [overflow census (4) | CS_SLICES column-sum
  // slices of 3 H | overflow H x H pair] (ES3C)
  // (ES3C: + CS_SLICES slices of H, the singleton states' sums of q of the kappa route)
  c->pre_n = (model == EVOAMD_MODEL_SSSC) ? 4 + (i64)CS_SLICES * 4 * H : 4 + (i64)BSC_CS_SLICES * H;
  c->ovf_n = c->pre_n + ((model == EVOAMD_MODEL_SSSC) ? 2 * (i64)H * H : 0);
}

// What belongs to the previous geometry and is rebuilt on demand (or by the groups below where this one needs it).
static void configure_drop(evoamd_ctx *c) {
  // masks / reconstructions: their buffers are N x D of THAT shard
  for (DevBuf<uint8_t> *b : {&c->mask_infr, &c->mask_x, &c->keep_x, &c->row_any}) b->reset();
  c->Yrec.reset();
  // the general device EA, sized by the geometry (evoamd_evolve_states)
  c->cand_raw.reset();
  c->dupold.reset();
  c->gen_start.reset();
  // W^T is sized by (H, D) of the geometry it was built for (ES3C: evoamd_upload_masks, derive_from_theta,
  // compute_reconstruction; EBSC allocates it below) -- never reused across a configure: a larger D would write past its end
  c->tmpWt.reset();
  c->Wt.reset();
  c->init_scratch.reset();
  c->seed_gpt.reset();
  c->seed_rows.reset();
  // the posterior samples of the previous geometry
  c->ps_slot.reset();
  c->ps_status.reset();
  c->ps_s.reset();
  c->ps_z.reset();
  c->ps_y.reset();
  made_posterior_samples(c, -1);
  // ... the inputs and outputs of evoamd_predictive_score (N x D of that geometry; nothing of them is handed out later)
  c->pscore_y.reset();
  c->pscore_q.reset();
  c->pscore_d.reset();
  c->pscore_i.reset();
  c->pscore_list.reset();
  // ... and the importance draws of evoamd_loglik_estimate
  c->lle_d.reset();
  c->lle_keep_d.reset();
  c->lle_rho.reset();
  c->lle_hash.reset();
  c->lle_i.reset();
  c->lle_flags.reset();
  c->lle_keep_s.reset();
  c->lle_keep_in.reset();
  made_loglik_draws(c, -1);
  // ... and the chains of evoamd_ais_loglik
  c->ais_d.reset();
  c->ais_i.reset();
  c->ais_s.reset();
  c->ais_nf.reset();
  // ... and of evoamd_ais_posterior
  c->aisp_d.reset();
  c->aisp_rows.reset();
  c->aisp_i.reset();
  c->aisp_s.reset();
  c->aisp_nf.reset();
  c->huge.reset();
  c->huge_ctl.reset();
  c->huge_slots = c->huge_kc = 0;
  for (DevBuf<float> *b : {&c->Yf, &c->Ytf, &c->Wf, &c->Bf, &c->Esf}) b->reset();
  c->Yt.reset();
}

static int configure_alloc_common(evoamd_ctx *c) {
  const size_t N = (size_t)c->N, D = (size_t)c->D, H = (size_t)c->H, S = (size_t)c->S, Cmax = (size_t)c->Cmax, HW = (size_t)c->HW;
  TRY(c->Y.alloc(N * c->ldY));
  TRY(c->yy.alloc(N));
  TRY(c->y2sum.alloc(D));
  TRY(c->states.alloc(N * S * HW));
  TRY(c->cand.alloc(N * Cmax * HW));
  if (H <= DIG_MAX_H) {
    TRY(c->dig.alloc(N * S));
    TRY(c->cand_dig.alloc(N * Cmax));
  } else {  // latent indices do not fit the digest's 14-bit slots: every kernel takes its word path
    c->dig.reset();
    c->cand_dig.reset();
  }
  TRY(c->lpj.alloc(N * c->L));
  TRY(c->lpj_alt.alloc(N * c->L));
  TRY(c->cand_lpj.alloc(N * Cmax));
  TRY(c->cand_counts.alloc(N));
  TRY(c->flags.alloc(3 * N));
  TRY(c->rowmax.alloc(N));
  TRY(c->rowsum.alloc(N));
  TRY(c->partial.alloc((size_t)3 * cdiv(c->N, 4)));
  TRY(c->partial2.alloc(cdiv(c->N, 4)));
  TRY(c->diag.alloc(H));
  // (the bool staging area, N x max(S, Cmax) x H bytes at most, grows on demand)
  TRY(c->W.alloc(D * H));
  TRY(c->tmpA.alloc(H * H));
  TRY(c->tmpB.alloc(H * H));
  TRY(c->tmpC.alloc(H * H));
  // two ping-pong H x H partners | pivoted path: D, Pn (2 x H x 32 each), ipiv, perm (unblocked,
  // H > 1024: colp | rowp | perm in the same place) | SPD path: Pinv (2 x 2 x 256), diag (2 x H)
  TRY(c->gjwork.alloc(2 * H * H + 132 * H + 1040 + 4 * GJS32 * GJS32));  // + pivot inverses of the 32-column path
  TRY(c->G.alloc(H * H));
  TRY(c->acc_base.alloc((size_t)c->ovf_n + c->acc_n + DP_COUNT));  // [... |] packed accumulator, then the scalar block (one D2H)
  c->census = c->acc_base;
  c->acc = c->acc_base + c->ovf_n;
  c->dpar = c->acc + c->acc_n;
  TRY(c->err.alloc(8));
  c->sing_gen = c->err + 4;
  // Y^T for B = Y W on the 128-tile kernel (measured: pays at H = 1024, D = 256 -- c5 2.07 -> 1.90 ms --, equal at H = 512,
  // slower at H = 256 / D = 64 where a tile has four K slabs; option value 2 forces it from H = 128 on for the tests).
  // Optional: the row-major product serves.
  if (!c->f32 && c->b_tn_opt && c->N >= 8192 && (c->H % 2) == 0 &&
      ((c->H >= 768 && c->D >= 128) || (c->b_tn_opt == 2 && c->H >= 128 && c->D >= 32))) {
    c->ldYt = ((c->N + 3) / 4) * 4;
    (void)c->Yt.try_alloc(D * c->ldYt);
  }
  return 0;
}

static int configure_alloc_ebsc(evoamd_ctx *c) {
  const size_t N = (size_t)c->N, D = (size_t)c->D, H = (size_t)c->H;
  TRY(c->Es_own.alloc(c->f32 ? 1 : N * H));
  c->Es = c->Es_own;
  TRY(c->Wt.alloc(H * D));
  TRY(c->Bm.alloc(c->f32 ? 1 : N * H));
  if (c->f32) {
    c->ldYt = ((c->N + 3) / 4) * 4;
    TRY(c->Yf.alloc(N * D));
    TRY(c->Ytf.alloc(D * c->ldYt));
    TRY(c->Wf.alloc(D * H));
    TRY(c->Bf.alloc(N * H));
    TRY(c->Esf.alloc(N * H));
  }
  return 0;
}

static int configure_alloc_es3c(evoamd_ctx *c) {
  const size_t N = (size_t)c->N, H = (size_t)c->H;
  c->Es_own.reset();
  c->Es = c->Y + c->D;  // lives inside c->Y
  TRY(c->Psi.alloc(H * H));
  TRY(c->GP.alloc(H * H));
  TRY(c->DG.alloc(H));
  TRY(c->D1.alloc(H));
  TRY(c->PT.alloc(H * H));
  TRY(c->Bm.alloc(N * H));
  TRY(c->mus.alloc(H));
  TRY(c->pilbar_v.alloc(H));
  TRY(c->pies.alloc(H));
  TRY(c->rowF.alloc(N));
  TRY(c->rowcnt.alloc(N));
  TRY(c->defer.alloc(2 * (N + 1) + 2));  // two lists of N datapoints, each with its counter behind it; + the reduce kernel's arrival counter
  TRY(c->fpart.alloc((size_t)3 * R3_THREADS));
  if (c->H > SSSC_KCAP) {
    // the reference evaluates a state with any number of active latents (sssc.py:261-324); above SSSC_KCAP the k x k
    // system does not fit a CU's LDS and the wavefront kernel works in one of these slots (at most 16, at most 256 MB)
    const size_t slot = big_slot_doubles(c->H);
    c->huge_kc = c->H;
    c->huge_slots = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)256 << 20) / (slot * sizeof(double))));
    TRY(c->huge.alloc(slot * (size_t)c->huge_slots));
    TRY(c->huge_ctl.alloc((size_t)c->huge_slots));
  }
  return 0;
}

// ES3C: the overflow lists of a batch of N x max(S, Cmax) pairs and the census lists of the N x S resident states
static int configure_alloc_lists(evoamd_ctx *c) {
  const size_t words = list_cap(c->N * (i64)std::max(c->S, c->Cmax)) * LIST_SHARDS;
  TRY(c->list1.alloc(words));
  TRY(c->list2.alloc(words));
  TRY(c->list3.alloc(words));
  TRY(c->list_n.alloc(4 * LIST_SHARDS));
  c->clist.reset();
  c->clist_n.reset();
  c->ovf_rec.reset();
  if (c->census_opt) {
    TRY(c->clist.alloc(3 * list_cap(c->N * (i64)c->S) * LIST_SHARDS));
    TRY(c->clist_n.alloc(4 * LIST_SHARDS));
    TRY(c->ovf_rec.alloc((size_t)c->N * c->S));
  }
  // the kappa records, where the route can run at all (optional: without them the passes take the table route)
  c->kap.reset();
  c->cand_kap.reset();
  if (c->census_opt && kappa_wanted(c) && c->dig && (c->H % 2) == 0 && !c->sssc_prec32 &&
      (size_t)(4 * 2 + 4) * c->H * sizeof(double) <= 150 * 1024) {
    if (!c->kap.try_alloc((size_t)c->N * c->S) || !c->cand_kap.try_alloc((size_t)c->N * c->Cmax)) {
      c->kap.reset();
      c->cand_kap.reset();
    }
  }
  return 0;
}

static int configure_alloc_host(evoamd_ctx *c) {
  const size_t par_n = (size_t)c->D * c->H + (size_t)c->H * c->H + 3 * (size_t)c->H;
  if (!c->h_err) TRY(c->h_err.alloc(4));
  if (!c->h_dpar) TRY(c->h_dpar.alloc(DP_COUNT + 8));
  TRY(c->h_acc.alloc((size_t)c->acc_n + DP_COUNT));
  TRY(c->h_par.alloc(par_n));
  c->h_theta_dev = nullptr;
  TRY(c->h_theta.alloc(par_n + MAILBOX_HDR, hipHostMallocCoherent | hipHostMallocMapped));
  memset(c->h_theta, 0, MAILBOX_HDR * sizeof(double));
  HIP_TRY(hipHostGetDevicePointer((void **)&c->h_theta_dev, c->h_theta, 0));
  if (!c->mbox_counter) {
    TRY(c->mbox_counter.alloc(1));
    HIP_TRY(hipMemset(c->mbox_counter, 0, sizeof(unsigned)));
  }
  return 0;
}

static int configure_clear(evoamd_ctx *c) {
  auto zero = [&](auto &b) { return hipMemsetAsync(b.get(), 0, b.size() * sizeof(*b.get()), c->stream); };
  if (c->huge_ctl) HIP_TRY(zero(c->huge_ctl));
  if (c->Yt) HIP_TRY(zero(c->Yt));
  if (c->f32) HIP_TRY(zero(c->Ytf));
  if (c->model == EVOAMD_MODEL_SSSC) {
    HIP_TRY(zero(c->defer));
    if (c->clist_n) HIP_TRY(zero(c->clist_n));
  }
  HIP_TRY(zero(c->Y));
  HIP_TRY(zero(c->flags));
  HIP_TRY(zero(c->cand_counts));
  HIP_TRY(zero(c->acc_base));
  HIP_TRY(zero(c->err));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_configure(evoamd_ctx *c, int model, int64_t N, int D, int H, int S, int S_perm,
                                int Cmax) {
  REQUIRE(c, "ctx is NULL");
  c->configured = false;  // until the last line: a configure that fails, at whichever stage, leaves a context that answers "configure first"
  TRY(configure_validate(c, model, N, D, H, S, S_perm, Cmax));
  HIP_TRY(hipSetDevice(c->device));
  configure_geometry(c, model, N, D, H, S, S_perm, Cmax);
  configure_drop(c);
  TRY(configure_alloc_common(c));
  if (model == EVOAMD_MODEL_BSC) {
    TRY(configure_alloc_ebsc(c));
  } else {
    TRY(configure_alloc_es3c(c));
    TRY(configure_alloc_lists(c));
  }
  TRY(alloc_pair_bins(c, c->bins_scale));
  TRY(configure_alloc_host(c));
  TRY(configure_clear(c));
  on_configure(c);
  c->configured = true;
  return 0;
}

extern "C" int evoamd_upload_data(evoamd_ctx *c, const double *Y) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(Y, "Y is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy2DAsync(c->Y, (size_t)c->ldY * sizeof(double), Y, (size_t)c->D * sizeof(double),
                           (size_t)c->D * sizeof(double), (size_t)c->N, hipMemcpyHostToDevice, c->stream));
  row_sqnorm_kernel<<<cdiv(c->N, 4), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->yy);
  HIP_TRY(hipMemsetAsync(c->y2sum, 0, (size_t)c->D * sizeof(double), c->stream));
  {
    launch_colsum<true>(c, c->Y, c->ldY, c->N, c->D, c->y2sum);
  }
  if (c->Yt)
    transpose_to_f64_kernel<<<dim3(cdiv(c->N, 32), cdiv(c->D, 32)), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->Yt, c->ldYt);
  if (c->f32) {  // float copies for the two long contractions: Y (N,D) and Y^T (D,N)
    to_f32_kernel<<<cdiv(c->N * (i64)c->D, 256), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->Yf, c->D);
    transpose_to_f32_kernel<<<dim3(cdiv(c->N, 32), cdiv(c->D, 32)), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->Ytf,
                                                                                       c->ldYt);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_data_uploaded(c);
  return 0;
}

extern "C" int evoamd_upload_masks(evoamd_ctx *c, const uint8_t *x_infr, const uint8_t *x) {
  REQUIRE(c && c->configured && c->have_data, "configure and upload_data first");
  REQUIRE(!(c->f32 && x_infr), "incomplete data is not available in the float32 mode");
  HIP_TRY(hipSetDevice(c->device));
  c->keep_differs = x_infr && x && memcmp(x, x_infr, (size_t)c->N * c->D) != 0;
  if (!x_infr) {  // back to complete data (upload_data again restores entries that were zeroed)
    c->mask_infr.reset();
    c->mask_x.reset();
    on_masks_changed(c, /*present=*/false);
    return 0;
  }
  const size_t nd = (size_t)c->N * c->D;
  TRY(c->mask_infr.alloc(nd));
  TRY(c->mask_x.alloc(nd));
  TRY(c->Yrec.alloc(nd));
  TRY(c->row_any.alloc((size_t)c->N));
  HIP_TRY(hipMemcpyAsync(c->mask_infr, x_infr, nd, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->mask_x, x ? x : x_infr, nd, hipMemcpyHostToDevice, c->stream));
  // missing entries (NaN in the reference's data) become zeros: they then drop out of ||y_obs||^2
  mask_apply_kernel<<<cdiv((i64)nd, 256), 256, 0, c->stream>>>(c->Y, c->ldY, c->mask_infr, c->N, c->D);
  if (c->Yt)  // B = Y W is formed from Y^T where it exists: it must hold the zeros too (evoamd_seed_states_ex reads that B)
    transpose_to_f64_kernel<<<dim3(cdiv(c->N, 32), cdiv(c->D, 32)), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->Yt, c->ldYt);
  row_sqnorm_kernel<<<cdiv(c->N, 4), 256, 0, c->stream>>>(c->Y, c->ldY, c->N, c->D, c->yy);
  patches_row_any_kernel<<<cdiv(c->N, 4), 256, 0, c->stream>>>(c->mask_infr, c->N, c->D, c->row_any);
  HIP_TRY(hipMemsetAsync(c->y2sum, 0, (size_t)c->D * sizeof(double), c->stream));
  launch_colsum<true>(c, c->Y, c->ldY, c->N, c->D, c->y2sum);
  if (c->model == EVOAMD_MODEL_SSSC) {  // W^T (H, D) for the per-datapoint Gram blocks
    if (!c->Wt) TRY(c->Wt.alloc((size_t)c->H * c->D));
    if (c->have_params)
      transpose_kernel<<<cdiv((i64)c->H * c->D, 256), 256, 0, c->stream>>>(c->W, c->D, c->H, c->Wt);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_masks_changed(c, /*present=*/true);
  return 0;
}

extern "C" int evoamd_set_reliable_fraction(evoamd_ctx *c, double reliable_per_datapoint) {
  REQUIRE(c, "ctx is NULL");
  c->rel_frac = reliable_per_datapoint;
  return 0;
}

extern "C" int evoamd_upload_yrec(evoamd_ctx *c, const double *y_rec) {
  REQUIRE(c && c->configured && c->mask_infr && y_rec, "upload_masks first");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->Yrec, y_rec, (size_t)c->N * c->D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_yrec_uploaded(c);
  return 0;
}

static int pack_to_device(evoamd_ctx *c, const uint8_t *host_bool, i64 nstates, u64 *dst) {
  const size_t bytes = (size_t)nstates * c->H;
  TRY(c->stage.ensure(c, bytes));
  HIP_TRY(hipMemcpyAsync(c->stage, host_bool, bytes, hipMemcpyHostToDevice, c->stream));
  pack_states_kernel<<<cdiv(nstates * c->HW, 256), 256, 0, c->stream>>>(c->stage, dst, nstates, c->H, c->HW);
  if (dst == c->states) on_kn_changed(c, KN_BY_CALLER);
  u64 *dg = dst == c->states ? c->dig : dst == c->cand ? c->cand_dig : nullptr;
  if (dg) digest_kernel<<<cdiv(nstates, 256), 256, 0, c->stream>>>(dst, dg, nstates, c->HW);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int evoamd_upload_states(evoamd_ctx *c, const uint8_t *ss_bool) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(ss_bool, "ss is NULL");
  HIP_TRY(hipSetDevice(c->device));
  TRY(pack_to_device(c, ss_bool, c->N * (i64)c->S, c->states));
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_kn_complete(c);
  return 0;
}

extern "C" int evoamd_download_states(evoamd_ctx *c, uint8_t *ss_bool) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(ss_bool, "ss is NULL");
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  const i64 ns = c->N * (i64)c->S;
  TRY(c->stage.ensure(c, (size_t)ns * c->H));
  unpack_states_kernel<<<cdiv(ns * c->H, 256), 256, 0, c->stream>>>(c->states, c->stage, ns, c->H, c->HW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ss_bool, c->stage, (size_t)ns * c->H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// K^n rows [n0, n0 + n) as np.packbits makes them: (n, S, ceil(H/8)) bytes, latent h in byte h/8 at bit 7-(h%8).
extern "C" int evoamd_upload_states_packed(evoamd_ctx *c, const uint8_t *packed, int64_t n0, int64_t n) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(packed && n0 >= 0 && n > 0 && n0 + n <= c->N, "bad row range");
  HIP_TRY(hipSetDevice(c->device));
  const int PB = (c->H + 7) / 8;
  const i64 ns = n * (i64)c->S;
  const size_t bytes = (size_t)ns * PB;
  TRY(c->stage.ensure(c, bytes));
  HIP_TRY(hipMemcpyAsync(c->stage, packed, bytes, hipMemcpyHostToDevice, c->stream));
  u64 *dst = c->states + (size_t)n0 * c->S * c->HW;
  words_from_packbits_kernel<<<cdiv(ns * c->HW, 256), 256, 0, c->stream>>>(c->stage, dst, ns, PB, c->HW, c->H);
  if (c->dig) digest_kernel<<<cdiv(ns, 256), 256, 0, c->stream>>>(dst, c->dig + (size_t)n0 * c->S, ns, c->HW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_kn_rows_uploaded(c, n0, n);
  return 0;
}

// K^n(0) drawn on the device (kernels_init.hpp; variational/utils.py:100-138 with a counter-based stream), or -- exact
// E-steps -- the caller's state table copied to every datapoint.
extern "C" int evoamd_init_states(evoamd_ctx *c, double p_init, uint64_t seed, int max_rounds, const uint8_t *table_packed) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(max_rounds >= 1 && max_rounds <= 65536, "evoamd_init_states: max_rounds must be in [1, 65536]");
  REQUIRE(!(c->bg_unit && c->S_perm), "evoamd_init_states: no permanent all-zero state with the background unit (variational/utils.py:42-47)");
  REQUIRE(c->H - c->bg_unit >= 1, "evoamd_init_states: no latent varies");
  HIP_TRY(hipSetDevice(c->device));
  const int S = c->S, HW = c->HW;
  if (table_packed) {
    const int Hv = c->H - c->bg_unit;
    REQUIRE(Hv < 12 && S + c->S_perm == (1 << Hv),
            "evoamd_init_states: a state table means exact E-steps, S + S_perm == 2^Hv with Hv < 12 (variational/utils.py:55)");
  }
  if (table_packed) {  // exact mode: (S, ceil(H/8)) packbits rows -> words behind them in the staging area -> every datapoint
    const int PB = (c->H + 7) / 8;
    const size_t off = (((size_t)S * PB + 7) / 8) * 8;
    TRY(c->stage.ensure(c, off + (size_t)S * HW * sizeof(u64)));
    u64 *table = (u64 *)(c->stage + off);
    HIP_TRY(hipMemcpyAsync(c->stage, table_packed, (size_t)S * PB, hipMemcpyHostToDevice, c->stream));
    SpanGuard g(c, KID_INIT_STATES);
    words_from_packbits_kernel<<<cdiv((i64)S * HW, 256), 256, 0, c->stream>>>(c->stage, table, S, PB, HW, c->H);
    init_states_tile_kernel<<<cdiv(c->N * (i64)S, 256), 256, 0, c->stream>>>(table, c->states, c->dig, c->N, S, HW);
  } else {
    InitArgs a;
    a.states = c->states;
    a.dig = c->dig;
    a.scratch = nullptr;
    a.err = c->err + INIT_ERR_WORD;
    a.N = c->N;
    a.S = S;
    a.S_perm = c->S_perm;
    a.H = c->H;
    a.Hv = c->H - c->bg_unit;
    a.HW = HW;
    a.max_rounds = max_rounds;
    a.seed = seed;
    a.p0 = p_init > 0.0 ? p_init : 1.0 / (double)c->H;
    const size_t wave_words = 2 * (size_t)(HW + 1) * S;  // candidates and held set, each HW word rows + the hash row
    int W = 4;
    while (W > 1 && W * wave_words * sizeof(u64) > 150 * 1024) W >>= 1;
    const bool lds_fits = W * wave_words * sizeof(u64) <= 150 * 1024;
    REQUIRE(c->init_home != 0 || lds_fits, "init_states_home 0 (LDS): the round state of one wavefront does not fit");
    const bool lds_home = c->init_home < 0 ? lds_fits : c->init_home == 0;
    on_kn_init_begun(c);
    HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(int), c->stream));
    if (lds_home) {
      const unsigned grid = (unsigned)std::min<i64>(cdiv(c->N, W), (i64)c->n_cu * 64);
      SpanGuard g(c, KID_INIT_STATES);
      init_states_kernel<true><<<grid, 64 * W, (size_t)W * wave_words * sizeof(u64), c->stream>>>(a);
    } else {  // slots of global memory, one per wave of a resident-sized grid (at most 256 MB)
      W = 4;
      i64 grid = std::min<i64>(cdiv(c->N, W), (i64)c->n_cu * 2);
      while (grid > 1 && (size_t)grid * W * wave_words * sizeof(u64) > ((size_t)256 << 20)) grid >>= 1;
      const size_t need = (size_t)grid * W * wave_words;
      TRY(c->init_scratch.ensure(c, need));
      a.scratch = c->init_scratch;
      SpanGuard g(c, KID_INIT_STATES);
      init_states_kernel<false><<<(unsigned)grid, 64 * W, 0, c->stream>>>(a);
    }
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "init_states");
    HIP_TRY(hipMemcpyAsync(c->h_err, a.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_err[0] & INIT_ERR_CAP) {
      HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(int), c->stream));
      return fail(EVOAMD_E_INVALID,
                  "evoamd_init_states: a datapoint holds fewer than S = %d distinct states after max_rounds = %d rounds (the "
                  "round cap); K^n is not initialised -- shapes with S close to 2^H belong to the host function",
                  S, max_rounds);
    }
    on_kn_complete(c);
    return 0;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_kn_changed(c, KN_BY_CALLER);
  on_kn_complete(c);
  return 0;
}

extern "C" int evoamd_download_states_packed(evoamd_ctx *c, uint8_t *packed, int64_t n0, int64_t n) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(packed && n0 >= 0 && n > 0 && n0 + n <= c->N, "bad row range");
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  const int PB = (c->H + 7) / 8;
  const i64 ns = n * (i64)c->S;
  const size_t bytes = (size_t)ns * PB;
  TRY(c->stage.ensure(c, bytes));
  packbits_from_words_kernel<<<cdiv(ns * PB, 256), 256, 0, c->stream>>>(c->states + (size_t)n0 * c->S * c->HW, c->stage, ns,
                                                                         PB, c->HW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(packed, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_upload_lpj(evoamd_ctx *c, const double *lpj) {
  REQUIRE(c && c->configured, "configure first");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->lpj, lpj, (size_t)c->N * c->L * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_lpj_overwritten(c);
  made_lpj_rows(c);  // the caller's word for it, as for the states it uploads
  return 0;
}

extern "C" int evoamd_download_lpj(evoamd_ctx *c, double *lpj) {
  REQUIRE(c && c->configured, "configure first");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(lpj, c->lpj, (size_t)c->N * c->L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// dense helpers
// ---------------------------------------------------------------------------------------
// 16-byte row pieces need an even leading dimension and a 16-byte aligned base
static bool gemm_vec_ok(const double *p, int ld) { return (ld % 2) == 0 && ((uintptr_t)p % 16) == 0; }
static bool gemm_vec_ok_f32(const float *p, int ld) { return (ld % 4) == 0 && ((uintptr_t)p % 16) == 0; }

// Ct / ldct: C^T as well where the parameter-sized kernel runs; returns whether it was written
static bool launch_gemm_nn_raw(evoamd_ctx *c, const double *A, int lda, const double *B, int ldb, double *C, int ldc,
                               i64 M, int Nc, int K, double *Ct = nullptr, int ldct = 0, i64 route_M = 0) {
  // route_M: the rows of the larger product that these M rows are some of; above 1024 that product takes the kernel below,
  // and so does this one, with its order of summation
  if (M <= 1024 && Nc <= 1024 && K <= 1024) {  // parameter-sized: one wave per 16 x 16 block
    if (route_M <= 1024) {
      c->route = {EVOAMD_ROUTE_NN_SMALL, 16, 1, 0, 0, 0, 0, 0};
      gemm_nn_small_kernel<<<dim3(cdiv(Nc, 16), cdiv(M, 16)), 256, 0, c->stream>>>(A, lda, B, ldb, C, ldc, (int)M, Nc, K, Ct, ldct);
      return Ct != nullptr;
    }
  }
  const int gx = (int)cdiv(Nc, GEMM_BN), gy = (int)cdiv(M, GEMM_BM);
  const int rows_per_xcd = (gy + 7) / 8;
  const unsigned grid = (unsigned)(8 * rows_per_xcd * gx);
  const bool vec = gemm_vec_ok(A, lda) && gemm_vec_ok(B, ldb) && (K % 2) == 0 && (Nc % 2) == 0 && K >= 2 && Nc >= 2 && M >= 1;
  c->route = {vec ? EVOAMD_ROUTE_NN_VEC : EVOAMD_ROUTE_NN_SCALAR, GEMM_BM, 1, 0, 0, 0, 0, 0};
  if (vec)
    gemm_nn_f64<true><<<grid, 256, 0, c->stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, gx, gy, rows_per_xcd);
  else
    gemm_nn_f64<false><<<grid, 256, 0, c->stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, gx, gy, rows_per_xcd);
  return false;
}

// How a C = A^T B product runs, beyond its operands (launch_gemm_tn; launch_gemm_tn_f32 reads stream and spare).
struct GemmTnOpts {
  bool deterministic = false;  // no split-K atomics: the same operands give the same bits every time
  // sym_row0 >= 0: rows sym_row0 .. of C are X^T X (symmetric, Nc x Nc, sym_row0 a multiple of the
  // tile size): only its upper tiles are computed, the rest is mirrored
  int sym_row0 = -1;
  bool c_is_zero = false;   // C needs no memset in front of a split product
  bool accumulate = false;  // C += A^T B with the atomic epilogue whatever the split (C holds earlier blocks of the same
                            // product: the chunked statistics pass)
  bool mirror = true;       // false leaves the lower tiles of a symmetric block for a later call
  hipStream_t stream = nullptr;  // nullptr = the main stream; the statistics contraction runs on stream2
  int spare = 0;  // stream-K / grouped grid: workgroups per XCD left unlaunched (stats_contract_block: beside the Theta chain)
  double *diag = nullptr;  // where gram_small_kernel runs (gram_is_small) it writes diag(C) here on its way
};

// G = W^T W small enough for the one-wave-per-16x16-block kernel, which can leave diag(G) as well
static bool gram_is_small(int M, i64 K) { return M <= 512 && K <= 4096; }

// Workspace of the stream-K contractions: `segmax` 128 x 128 slabs per workgroup (a run of U / wpx units touches at
// most n_real / wpx + 2 tiles).  Returns nullptr (atomic epilogue) when it cannot be had.
static double *streamk_workspace(evoamd_ctx *c, unsigned wpx, i64 n_real, int *segmax) {
  *segmax = (int)(n_real / wpx) + 2;
  const size_t need = (size_t)8 * wpx * (size_t)*segmax * GEMM_T * GEMM_T;
  if (need > c->gemm_ws.size() && !c->gemm_ws.try_alloc(need)) return nullptr;
  return c->gemm_ws;
}

// C (M x Nc) = A^T B, K rows; C is zeroed first when K is split.
static int launch_gemm_tn(evoamd_ctx *c, const double *A, int lda, const double *B, int ldb, double *C, int ldc,
                          int M, int Nc, i64 K, const GemmTnOpts &o = GemmTnOpts()) {
  const bool deterministic = o.deterministic, c_is_zero = o.c_is_zero, accumulate = o.accumulate, mirror = o.mirror;
  int sym_row0 = o.sym_row0;
  const hipStream_t stream = o.stream ? o.stream : c->stream;
  if (deterministic && A == B && lda == ldb && M == Nc && sym_row0 < 0 && gram_is_small(M, K)) {
    // G = W^T W of the Theta update: one wave per 16 x 16 block (gram_small_kernel)
    SpanGuard g(c, KID_GEMM, stream);
    const int nb16 = (int)cdiv(M, 16);
    c->route = {EVOAMD_ROUTE_GRAM_SMALL, 16, 1, 0, 0, 0, 0, 0};
    gram_small_kernel<<<dim3(nb16, nb16), 256, 0, stream>>>(A, lda, (int)K, M, C, ldc, o.diag);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const bool vec = gemm_vec_ok(A, lda) && gemm_vec_ok(B, ldb) && (M % 2) == 0 && (Nc % 2) == 0 && M >= 2 && Nc >= 2;
  // long-K, wide outputs: 128 x 128 tiles (half the L2 traffic per flop)
  const bool big = vec && !deterministic && K >= 8192 && M >= 256 && Nc >= 256 &&
                   (sym_row0 < 0 || (sym_row0 % GEMM_T) == 0);
  const int T = big ? GEMM_T : GEMM_BM;
  if (sym_row0 >= 0 && (sym_row0 % T) != 0) sym_row0 = -1;
  const int gx = (int)cdiv(Nc, T), gy = (int)cdiv(M, T);
  const i64 tiles = (i64)gx * gy;
  // enough workgroups to fill the chip, at least 64 rows of K per chunk; the kernel spreads the K
  // chunks over the 8 XCDs, so a split uses a multiple of 8 chunks.  64-tiles: >= 512 workgroups;
  // 128-tiles (2 per CU, 64 per XCD): chunks per XCD chosen so that the last round of an XCD is
  // at least 90 % full
  i64 splits = 1;
  if (K >= 128 && !deterministic) {
    if (big) {
      // tiles that really run (the strictly lower tiles of a symmetric block exit at once)
      i64 real = tiles;
      if (sym_row0 >= 0) {
        const i64 ts = cdiv(Nc, T);
        real -= ts * (ts - 1) / 2;
      }
      // chunks per XCD: the fullest last round of the 64 resident workgroups of an XCD
      i64 per_xcd = 1;
      double best = 0.0;
      for (i64 pc = 1; pc <= 16; pc++) {
        // at least 512 rows of K per chunk: below that the ramp of the software pipeline and the atomic
        // epilogue of every extra chunk cost more than a fuller last round gains (K = 12500, 34 tiles:
        // 15 chunks per XCD 0.455 ms, 3 chunks 0.374 ms; tools/gemm_sweep.sh)
        if (pc > 1 && K / (8 * pc) < 512) break;
        const double eff = (double)(real * pc) / (64.0 * (double)cdiv(real * pc, 64));
        if (eff > best + 0.01) {
          best = eff;
          per_xcd = pc;
        }
      }
      // measured exception (tools/gemm_sweep.sh, 34 real tiles = the ES3C H = 512 contraction, K = 25k / 50k /
      // 100k): 8 chunks per XCD beat the fullest split by 5-7 % (2.44 vs 2.59 ms at K = 100k), and so do 16;
      // other counts between 5 and 15 do not.  The cause was not isolated (chunk count a multiple of the
      // XCD count in both winners); applied only in that multi-round regime.
      if (real > 24 && K / 64 >= 384) per_xcd = 8;
      if (c->gemm_per_xcd > 0) per_xcd = c->gemm_per_xcd;
      splits = 8 * per_xcd;
    } else {
      splits = (512 + tiles - 1) / tiles;
    }
    const i64 maxs = (K + 63) / 64;
    if (splits > maxs) splits = maxs;
    if (splits > 1) splits = ((splits + 7) / 8) * 8;
  }
  if (accumulate && splits < 8) splits = 8;  // the atomic epilogue needs the split decode (8 chunks, one per XCD)
  const int split = splits > 1;
  i64 kps = K;
  if (split) {
    kps = (K + splits - 1) / splits;
    kps = ((kps + GEMM_BK - 1) / GEMM_BK) * GEMM_BK;
    if (!c_is_zero && !accumulate) {
      // the product's own M x Nc region only: the columns Nc .. ldc of a wider C belong to the caller
      if (ldc == Nc)
        HIP_TRY(hipMemsetAsync(C, 0, (size_t)M * ldc * sizeof(double), stream));
      else
        HIP_TRY(hipMemset2DAsync(C, (size_t)ldc * sizeof(double), 0, (size_t)Nc * sizeof(double), (size_t)M, stream));
    }
  }
  const unsigned grid = (unsigned)(tiles * (split ? splits : 1));
  SpanGuard g(c, KID_GEMM, stream);
  if (!big) c->route = {vec ? EVOAMD_ROUTE_TN64_VEC : EVOAMD_ROUTE_TN64_SCALAR, T, (int)splits, 0, 0, 0, 0, 0};
  if (big && split && c->gemm_streamk) {
    // stream-K: one resident-sized grid, every XCD owns an eighth of K (option "gemm_streamk")
    i64 real = tiles;
    if (sym_row0 >= 0) {
      const i64 ts = cdiv(Nc, T);
      real -= ts * (ts - 1) / 2;
    }
    const i64 Kx = ((cdiv(K, 8) + GEMM_BK - 1) / GEMM_BK) * GEMM_BK;
    // forked beside the Theta-update chain (stats_compute): leave sk_spare slots per XCD to the chain's kernels
    const unsigned wpx = (unsigned)std::max(1, 2 * c->n_cu / 8 - o.spare);
    int segmax = 0;
    double *ws = c->gemm_ws_opt ? streamk_workspace(c, wpx, real, &segmax) : nullptr;
    // grouped split-K (gemm_f64.hpp): when whole chunks per tile fill the resident grid (>= 93 % of its slots) and a
    // chunk is long enough for the pipeline ramp
    const i64 J = (i64)8 * wpx / real;
    const bool grouped = ws && c->gemm_grouped && J >= 2 && real * J * 100 >= (i64)8 * wpx * 93 && K / J >= 256;
    c->route = {grouped ? EVOAMD_ROUTE_TN128_GROUPED : EVOAMD_ROUTE_TN128_STREAMK, T, (int)splits, (int)J, (int)wpx, segmax, ws != nullptr, 0};
    if (grouped) {
      const i64 Kc = ((cdiv(K, J) + 2 * GEMM_BK - 1) / (2 * GEMM_BK)) * (2 * GEMM_BK);  // whole slab pairs: no padding slab, mask-free drain
      gemm_tn128_gk<double><<<8 * wpx, 256, GEMM128_LDS_BYTES, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, Kc, gx, gy,
                                                                            sym_row0, (int)real, (int)J, ws);
      gemm_gk_reduce_kernel<<<dim3((unsigned)real, GEMM_T * GEMM_T / 256), 256, 0, stream>>>(ws, C, ldc, M, Nc, gx, gy,
                                                                                               sym_row0, (int)real, (int)J);
    } else {
    gemm_tn128_sk_f64<<<8 * wpx, 256, GEMM128_LDS_BYTES, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, Kx, gx, gy, sym_row0,
                                                                       (int)real, ws, segmax);
    if (ws)
      gemm_sk_reduce_kernel<<<dim3((unsigned)real, GEMM_T * GEMM_T / 256), 256, 0, stream>>>(
          ws, segmax, C, ldc, M, Nc, K, Kx, gx, gy, sym_row0, (int)real, (int)wpx);
    }
  } else if (big) {
    c->route = {EVOAMD_ROUTE_TN128_SPLIT, T, (int)splits, 0, 0, 0, 0, 0};
    gemm_tn128_f64<<<grid, 256, GEMM128_LDS_BYTES, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, kps, gx, gy, split, sym_row0);
  } else if (vec)
    gemm_tn_f64<true><<<grid, 256, 0, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, kps, gx, gy, split, sym_row0);
  else
    gemm_tn_f64<false><<<grid, 256, 0, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, kps, gx, gy, split, sym_row0);
  if (sym_row0 >= 0 && mirror)
    mirror_lower_kernel<<<cdiv((i64)Nc * Nc, 256), 256, 0, stream>>>(C + (size_t)sym_row0 * ldc, Nc, ldc, T);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int launch_gemm_nn(evoamd_ctx *c, const double *A, int lda, const double *B, int ldb, double *C, int ldc,
                          i64 M, int Nc, int K) {
  SpanGuard g(c, KID_GEMM);
  launch_gemm_nn_raw(c, A, lda, B, ldb, C, ldc, M, Nc, K);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------
static int launch_B_f32(evoamd_ctx *c);

// C (M x Nc) = At^T B with the whole K per 128 x 128 tile: At (K x M) and B (K x Nc) are read in 16-byte pieces, so both
// need an even leading dimension, a 16-byte aligned base and (B) an even Nc; M may be odd when lda is rounded up past it
// (the piece across column M - 1 stays inside the row, the row it feeds is never stored).
static void launch_rows_f64(evoamd_ctx *c, const double *At, int lda, const double *B, int ldb, double *C, int ldc, int M,
                            int Nc, i64 K) {
  const int gx = (int)cdiv(Nc, GEMM_T), gy = (int)cdiv(M, GEMM_T);
  c->route = {EVOAMD_ROUTE_ROWS, GEMM_T, 1, 0, 0, 0, 0, 0};
  gemm_tn128_rows_f64<<<(unsigned)(8 * cdiv(gy, 8) * gx), 256, GEMM128_LDS_BYTES, c->stream>>>(At, lda, B, ldb, C, ldc, M, Nc,
                                                                                                K, gx, gy);
}

// B = Y W (N x H): float32 mode, or from Y^T on the 128-tile kernel (large N), or the 64-tile row-major product
static int launch_B(evoamd_ctx *c) {
  if (c->f32) return launch_B_f32(c);
  if (!c->Yt) return launch_gemm_nn(c, c->Y, c->ldY, c->W, c->H, c->Bm, c->H, c->N, c->H, c->D);
  SpanGuard g(c, KID_GEMM);
  launch_rows_f64(c, c->Yt, (int)c->ldYt, c->W, c->H, c->Bm, c->H, (int)c->N, c->H, c->D);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Everything the next E-step reads that depends on Theta: G = W^T W and diag(G) (EBSC) or the state-term tables (ES3C,
// one theta_gen stamp per build), W^T for ES3C on incomplete data, B = Y W where there is data; B_valid says whether B
// was built.  All on the main stream.  `updated`: Theta was written by the device update (theta_update_*), not uploaded --
// the ES3C update has formed G already (its trace term reads it), and the EBSC Gram kernel leaves diag(G) on its way
// where the parameter-sized kernel runs (an upload always launches extract_diag_kernel).
static int derive_from_theta(evoamd_ctx *c, bool updated) {
  const int H = c->H, D = c->D;
  drop_B(c);
  if (c->model == EVOAMD_MODEL_BSC && c->bsc_direct) return 0;  // the direct residual kernel reads W only
  GemmTnOpts gram;
  gram.deterministic = true;  // the same Theta gives the same G, tables and lpj bits every time
  if (c->model == EVOAMD_MODEL_SSSC) {
    if (!updated) {
      TRY(launch_gemm_tn(c, c->W, H, c->W, H, c->G, H, H, H, D, gram));
      DBG_SYNC(c, "derive_from_theta: G = W^T W");
    }
    if (c->mask_infr) {  // incomplete data: the wavefront kernel forms W_obs^T W_obs from W^T (sssc.py:276)
      if (!c->Wt) TRY(c->Wt.alloc((size_t)H * D));
      transpose_kernel<<<cdiv((i64)H * D, 256), 256, 0, c->stream>>>(c->W, D, H, c->Wt);
    }
    sssc_tables_kernel<<<cdiv((i64)H * H, 256), 256, 0, c->stream>>>(c->G, c->Psi, c->mus, c->pilbar_v, c->dpar, H, c->D1,
                                                                     c->PT, c->GP, c->DG, c->sing_gen, next_theta_stamp(c));
    DBG_SYNC(c, "derive_from_theta: tables");
  } else {
    const bool diag_rides = updated && gram_is_small(H, D);
    if (diag_rides) gram.diag = c->diag;
    TRY(launch_gemm_tn(c, c->W, H, c->W, H, c->G, H, H, H, D, gram));
    if (!diag_rides) extract_diag_kernel<<<cdiv(H, 256), 256, 0, c->stream>>>(c->G, H, c->diag);
  }
  HIP_TRY(hipGetLastError());
  if (c->have_data) {
    TRY(launch_B(c));  // B = Y W
    made_B(c);
  }
  return 0;
}

extern "C" int evoamd_set_params_bsc(evoamd_ctx *c, const double *W, double pi, double sigma, double *ljc) {
  REQUIRE(c && c->configured && c->model == EVOAMD_MODEL_BSC, "context is not configured for BSC");
  REQUIRE(W, "W is NULL");
  REQUIRE(!(c->f32 && c->bsc_direct), "the direct residual kernel is not available in the float32 mode");
  HIP_TRY(hipSetDevice(c->device));
  // bsc.py:111-121; incomplete data: the normaliser counts the reliable entries (bsc.py:113-118)
  c->ljc = c->H * log(1.0 - pi) - (c->rel_frac >= 0.0 ? c->rel_frac : (double)c->D) / 2.0 * log(2 * M_PI * sigma * sigma);
  if (ljc) *ljc = c->ljc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // pinned mirrors may still be in flight
  memset(c->h_dpar, 0, DP_COUNT * sizeof(double));
  c->h_dpar[DP_PRE1] = -1.0 / 2.0 / sigma / sigma;
  c->h_dpar[DP_PILBAR] = log(pi / (1.0 - pi));
  c->h_dpar[DP_LJC] = c->ljc;
  c->h_dpar[DP_PI] = pi;
  c->h_dpar[DP_SIGMA] = sigma;
  HIP_TRY(hipMemcpyAsync(c->dpar, c->h_dpar, DP_COUNT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // W^T on the host (H x D); tiny
  HIP_TRY(hipStreamSynchronize(c->stream));  // the pinned staging area may still be in flight
  double *wt = c->h_par;                      // D*H doubles
  for (int d = 0; d < c->D; d++)
    for (int h = 0; h < c->H; h++) wt[(size_t)h * c->D + d] = W[(size_t)d * c->H + h];
  HIP_TRY(hipMemcpyAsync(c->Wt, wt, (size_t)c->H * c->D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(wt, W, (size_t)c->D * c->H * sizeof(double));
  HIP_TRY(hipMemcpyAsync(c->W, wt, (size_t)c->D * c->H * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TRY(derive_from_theta(c, /*updated=*/false));
  on_theta_installed(c);
  return 0;
}

extern "C" int evoamd_set_params_sssc(evoamd_ctx *c, const double *W, const double *pies, const double *mus,
                                      const double *Psi, double sigma2, double *ljc) {
  REQUIRE(c && c->configured && c->model == EVOAMD_MODEL_SSSC, "context is not configured for SSSC");
  REQUIRE(W && pies && mus && Psi, "NULL parameter array");
  HIP_TRY(hipSetDevice(c->device));
  const int H = c->H, D = c->D;
  // sssc.py:340-353: sigma2 through long double, rounded back to double
  const long double s2 = (long double)sigma2;
  // precision = float32 (sssc.py:344-349): 1 / sigma2 and D log sigma2 pass through float32 -- values only, every
  // product that uses them is still formed in double (a float32 scalar times a float64 array is float64 in NumPy)
  const double s2inv = c->sssc_prec32 ? (double)(float)(1.0L / s2) : (double)(1.0L / s2);
  double l = 0.0;
  std::vector<double> pb(H);
  {
    // np.log(1.0 - pies).sum(): NumPy's pairwise summation differs from a left-to-right loop by
    // rounding only (|ljc| ~ H * 0.4); keep a compensated sum to stay below 1 ulp of the result
    long double acc = 0.0L;
    for (int h = 0; h < H; h++) {
      acc += (long double)log(1.0 - pies[h]);
      pb[h] = log(pies[h] / (1.0 - pies[h]));
    }
    l = (double)acc;
  }
  if (c->rel_frac >= 0.0) {  // sssc.py:352-357: the Gaussian normaliser counts the reliable entries
    l += (-log(2 * M_PI) - log(sigma2)) * c->rel_frac / 2.0;
  } else {
    l -= D / 2.0 * log(2 * M_PI);
    if (c->sssc_prec32) {
      const float ld = (float)D * (float)logl(s2);  // D * float32: a float32 product
      l -= (double)(0.5f * ld);
    } else {
      l -= 0.5 * (D * (double)logl(s2));
    }
  }
  c->ljc = l;
  if (ljc) *ljc = l;
  HIP_TRY(hipStreamSynchronize(c->stream));  // the pinned staging area may still be in flight
  {
    double *hw = c->h_par, *hpsi = hw + (size_t)D * H, *hmu = hpsi + (size_t)H * H, *hpb = hmu + H, *hpi = hpb + H;
    memcpy(hw, W, (size_t)D * H * sizeof(double));
    memcpy(hpsi, Psi, (size_t)H * H * sizeof(double));
    memcpy(hmu, mus, (size_t)H * sizeof(double));
    memcpy(hpb, pb.data(), (size_t)H * sizeof(double));
    memcpy(hpi, pies, (size_t)H * sizeof(double));
    memset(c->h_dpar, 0, DP_COUNT * sizeof(double));
    c->h_dpar[DP_S2INV] = s2inv;
    c->h_dpar[DP_SIGMA2] = sigma2;
    c->h_dpar[DP_LJC] = l;
    HIP_TRY(hipMemcpyAsync(c->dpar, c->h_dpar, DP_COUNT * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->pies, hpi, (size_t)H * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->W, hw, (size_t)D * H * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->Psi, hpsi, (size_t)H * H * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->mus, hmu, (size_t)H * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->pilbar_v, hpb, (size_t)H * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  TRY(derive_from_theta(c, /*updated=*/false));
  on_theta_installed(c);
  return 0;
}

// float32 mode: C (M x Nc double, zeroed by the caller) += A^T B with float A (K x M), B (K x Nc): the stream-K grid on
// v_mfma_f32_16x16x4_f32 with the f64 atomic epilogue; small outputs by the one-thread-per-element kernel.
static int launch_gemm_tn_f32(evoamd_ctx *c, const float *A, int lda, const float *B, int ldb, double *C, int ldc, int M, int Nc,
                              i64 K, const GemmTnOpts &o = GemmTnOpts()) {
  const hipStream_t stream = o.stream ? o.stream : c->stream;
  SpanGuard g(c, KID_GEMM, stream);
  if (M >= 128 && Nc >= 128 && K >= 2048 && (M % 4) == 0 && (Nc % 4) == 0 && gemm_vec_ok_f32(A, lda) && gemm_vec_ok_f32(B, ldb)) {
    const int gx = (int)cdiv(Nc, GEMM_T), gy = (int)cdiv(M, GEMM_T);
    const i64 Kx = ((cdiv(K, 8) + GEMM_BK - 1) / GEMM_BK) * GEMM_BK;
    const unsigned wpx = (unsigned)std::max(1, 2 * c->n_cu / 8 - o.spare);
    int segmax = 0;
    double *ws = c->gemm_ws_opt ? streamk_workspace(c, wpx, (i64)gx * gy, &segmax) : nullptr;
    const i64 real = (i64)gx * gy, J = (i64)8 * wpx / real;
    const bool grouped = ws && c->gemm_grouped && J >= 2 && real * J * 100 >= (i64)8 * wpx * 93 && K / J >= 256;  // see launch_gemm_tn
    c->route = {grouped ? EVOAMD_ROUTE_F32_GROUPED : EVOAMD_ROUTE_F32_STREAMK, GEMM_T, 8, (int)J, (int)wpx, segmax, ws != nullptr, 0};
    if (grouped) {
      const i64 Kc = ((cdiv(K, J) + 2 * GEMM_BK - 1) / (2 * GEMM_BK)) * (2 * GEMM_BK);
      gemm_tn128_gk<float><<<8 * wpx, 256, GEMM128_LDS_BYTES, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, Kc, gx, gy, -1,
                                                                           (int)real, (int)J, ws);
      gemm_gk_reduce_kernel<<<dim3((unsigned)real, GEMM_T * GEMM_T / 256), 256, 0, stream>>>(ws, C, ldc, M, Nc, gx, gy, -1,
                                                                                               (int)real, (int)J);
    } else {
      gemm_tn128_sk_f32<<<8 * wpx, 256, GEMM128_LDS_BYTES, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K, Kx, gx, gy, gx * gy,
                                                                         ws, segmax);
      if (ws)
        gemm_sk_reduce_kernel<<<dim3((unsigned)(gx * gy), GEMM_T * GEMM_T / 256), 256, 0, stream>>>(
            ws, segmax, C, ldc, M, Nc, K, Kx, gx, gy, -1, gx * gy, (int)wpx);
    }
  } else {
    c->route = {EVOAMD_ROUTE_F32_NAIVE, 0, 1, 0, 0, 0, 0, 0};
    gemm_tn_naive_f32<<<cdiv((i64)M * Nc, 256), 256, 0, stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// C (M x Nc float) = A B from the transposed copy At (K x M) on the f32 matrix cores where the 128-tile store kernel can
// read 16-byte pieces (leading dimensions multiples of 4, 16-byte aligned bases, Nc a multiple of 4: a piece of B that
// straddles column Nc - 1 would run into the next row, behind the last row out of the buffer), else one thread per
// element from the row-major A (M x K).
static void launch_rows_f32(evoamd_ctx *c, const float *At, int ldat, const float *A, int lda, const float *B, int ldb,
                            float *C, int ldc, i64 M, int Nc, int K) {
  if (Nc >= 128 && M >= 128 && (Nc % 4) == 0 && gemm_vec_ok_f32(At, ldat) && gemm_vec_ok_f32(B, ldb)) {
    const int gx = (int)cdiv(Nc, GEMM_T), gy = (int)cdiv(M, GEMM_T);
    c->route = {EVOAMD_ROUTE_ROWS_F32_STORE, GEMM_T, 1, 0, 0, 0, 0, 0};
    gemm_tn128_store_f32<<<(unsigned)gx * gy, 256, GEMM128_LDS_BYTES, c->stream>>>(At, ldat, B, ldb, C, ldc, (int)M, Nc, K, gx);
  } else {
    c->route = {EVOAMD_ROUTE_ROWS_F32_NAIVE, 0, 1, 0, 0, 0, 0, 0};
    gemm_nn_naive_f32<<<cdiv(M * (i64)Nc, 256), 256, 0, c->stream>>>(A, lda, B, ldb, C, ldc, M, Nc, K);
  }
}

// float32 mode: Wf <- W, then Bf = Y W as (Y^T)^T Wf on the f32 matrix cores (whole K = D per 128 x 128 tile)
static int launch_B_f32(evoamd_ctx *c) {
  SpanGuard g(c, KID_GEMM);
  to_f32_kernel<<<cdiv((i64)c->D * c->H, 256), 256, 0, c->stream>>>(c->W, c->H, c->D, c->H, c->Wf, c->H);
  launch_rows_f32(c, c->Ytf, (int)c->ldYt, c->Yf, c->D, c->Wf, c->H, c->Bf, c->H, c->N, c->H, c->D);
  HIP_TRY(hipGetLastError());
  return 0;
}

// B = Y W depends on both the data and Theta; recompute it if either arrived later.
static int ensure_B(evoamd_ctx *c) {
  if (c->B_valid || (c->model == EVOAMD_MODEL_BSC && c->bsc_direct)) return 0;
  TRY(launch_B(c));
  DBG_SYNC(c, "B = Y W");
  made_B(c);
  return 0;
}

// ---------------------------------------------------------------------------------------
// lpj launches
// ---------------------------------------------------------------------------------------
struct Batch {
  const u64 *states;
  const int *counts;
  const double *Y;   // BSC: datapoints (N rows)
  const double *Bm;  // SSSC
  const double *yy;
  i64 N;
  int C, shared;
  double *out;
  int ldo, col0;
  unsigned *flags;
  int kid;
  int tag;  // 0 resident K^n, 1 candidate batch, 2 anything else: names the kernel instantiations (batch_hints)
  const uint8_t *mask = nullptr;  // EBSC incomplete data: x_infr rows of this batch's datapoints
};

// digests exist for the two resident state arrays only
static const u64 *dig_for(const evoamd_ctx *c, const u64 *states) {
  if (!c->use_digest) return nullptr;
  return states == c->states ? c->dig : states == c->cand ? c->cand_dig : nullptr;
}

static int launch_bsc_lpj(evoamd_ctx *c, const Batch &b) {
  if (!c->bsc_direct && b.tag != 2 && !b.mask) {  // masked data: per-datapoint Gram matrices -> direct form
    const i64 total = b.N * (i64)b.C;
    unsigned grid = cdiv(total, 256);
    // float32 mode: the batches over the resident data read the float B (per-datapoint calls bring their own double row)
    const int bf32 = (c->f32 && b.Bm == c->Bm) ? 1 : 0;
    const void *bmat = bf32 ? (const void *)c->Bf : (const void *)b.Bm;
    SpanGuard g(c, b.kid);
    // second-generation kernel (register state words, B rows in LDS) when the shape allows it
    const int rows_cap = 512 / b.C + 2;
    const size_t lds = (size_t)rows_cap * c->H * sizeof(double);
    const bool hw_ok = c->HW == 1 || c->HW == 2 || c->HW == 4 || c->HW == 8 || c->HW == 16;
    const u64 *dg = b.shared ? nullptr : dig_for(c, b.states);  // with digests the word template is unused
    if (!b.shared && (hw_ok || dg) && (c->H % 2) == 0 && lds <= 40 * 1024) {
      const unsigned g2 = cdiv(total, 512);
#define GRAM2(TAG, HWT)                                                                                      \
  bsc_lpj_gram2_kernel<TAG, HWT><<<g2, 512, lds, c->stream>>>(b.states, b.counts, bmat, b.yy, c->G, b.N, b.C, c->H, \
                                                              c->HW, c->dpar, b.out, b.ldo, b.col0, b.flags, c->err, dg, bf32, c->diag)
#define GRAM2_HW(TAG)                    \
  switch (c->HW) {                       \
    case 1: GRAM2(TAG, 1); break;        \
    case 2: GRAM2(TAG, 2); break;        \
    case 4: GRAM2(TAG, 4); break;        \
    case 8: GRAM2(TAG, 8); break;        \
    default: GRAM2(TAG, 16); break;      \
  }
      if (b.tag == 0) {
        GRAM2_HW(0)
      } else {
        GRAM2_HW(1)
      }
#undef GRAM2_HW
#undef GRAM2
      HIP_TRY(hipGetLastError());
      return 0;
    }
#define GRAM_LAUNCH(TAG)                                                                                       \
  bsc_lpj_gram_kernel<TAG><<<grid, 256, 0, c->stream>>>(b.states, b.counts, bmat, b.yy, c->G, b.N, b.C, b.shared, \
                                                        c->H, c->HW, c->dpar, b.out, b.ldo, b.col0, b.flags, c->err, dg, bf32, c->diag)
    if (b.tag == 0)
      GRAM_LAUNCH(0);
    else
      GRAM_LAUNCH(1);
#undef GRAM_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const int nchunk = (b.C + BSC_CHUNK - 1) / BSC_CHUNK;
  const unsigned grid = cdiv(b.N * nchunk, 4);
  SpanGuard g(c, b.kid);
#define BSC_LAUNCH(R)                                                                                     \
  bsc_lpj_kernel<R><<<grid, 256, 0, c->stream>>>(b.Y, c->Wt, b.states, b.counts, b.N, b.C, b.C, b.shared, \
                                                  c->D, c->HW, c->dpar, b.out, b.ldo, b.col0, b.flags, c->err, b.mask)
  if (c->D <= 64)
    BSC_LAUNCH(1);
  else if (c->D <= 128)
    BSC_LAUNCH(2);
  else
    BSC_LAUNCH(4);
#undef BSC_LAUNCH
  HIP_TRY(hipGetLastError());
  return 0;
}

static SsscArgs sssc_args(evoamd_ctx *c, const Batch &b) {
  SsscArgs a = {};
  a.states = b.states;
  a.dig = b.shared ? nullptr : dig_for(c, b.states);
  a.counts = b.counts;
  a.Bm = b.Bm;
  a.yy = b.yy;
  a.GP = c->GP;
  a.DG = c->DG;
  a.D1 = c->D1;
  a.PT = c->PT;
  a.mus = c->mus;
  a.pil_bar = c->pilbar_v;
  a.s2inv = 0.0;
  a.dpar = c->dpar;
  a.N = b.N;
  a.C = b.C;
  a.shared = b.shared;
  a.H = c->H;
  a.HW = c->HW;
  a.lpj_out = b.out;
  a.ldo = b.ldo;
  a.col0 = b.col0;
  a.flags = b.flags;
  a.err = c->err;
  a.sing_gen = c->sing_gen;
  a.gen = c->theta_gen;
  a.screen = c->sing_screen;
  a.huge = c->huge;
  a.huge_ctl = c->huge_ctl;
  a.huge_slots = c->huge_slots;
  a.huge_kc = c->huge_kc;
  a.mask = b.mask;
  a.Wt = c->Wt;
  a.D = c->D;
  return a;
}

static size_t big_lds(int kc) { return (size_t)(4 * kc * kc + 5 * kc) * sizeof(double) + (size_t)kc * sizeof(int); }

// What the caller of an ES3C pass knows about its states beyond the context, and how much of the pass it wants.
// The overflow counts of the last statistics pass (res_need / res_cnt, valid while need_known) describe
//   known_tag 0: exactly these states (the pass over K^n itself): the levels and grids they say;
//   known_tag 1: these states' parents -- the counted K^n plus candidates (a candidate batch, the final K^n of the
//                statistics pass, a prefetched pass over a K^n whose counts the host has not seen yet): grids sized
//                like children; with one_bit, every state not counted differs from a counted one in one bit, so it can
//                exceed a level only if some counted state exceeded the level below;
//   known_tag 2: nothing: every level, worst-case grids.
// The kernel instantiations keep the name of the batch (Batch::tag) whatever is known about it.
struct LevelHints {
  int known_tag = 2;
  bool one_bit = false;
  double scale = 1.0;        // share of the counted datapoints the launches cover (a block of a chunked statistics pass)
  bool levels_only = false;  // census route: no main kernel (the fused E-step evaluates <= 2 latents itself)
};

// Hints of the lpj pass over a batch.  prefetched: enqueued before the host has seen the counts of the K^n it evaluates
// (they still describe the previous one), so a pass over K^n chooses its levels like a candidate batch.
static LevelHints batch_hints(const evoamd_ctx *c, int tag, bool prefetched = false) {
  LevelHints lv;
  const bool stale = tag == 0 && prefetched;
  lv.known_tag = stale ? 1 : tag;
  lv.one_bit = stale || (tag == 1 && c->cand_from_device);
  return lv;
}

// Overflow levels (3..4, 5..8, above 8 latents) a pass needs.
static void levels_for(const evoamd_ctx *c, const LevelHints &lv, bool need[3]) {
  need[0] = need[1] = need[2] = true;
  if (!c->need_known) return;
  if (lv.known_tag == 0) {
    need[0] = c->res_need[0];
    need[1] = c->res_need[1];
    need[2] = c->res_need[2];
  } else if (lv.known_tag == 1 && lv.one_bit) {
    need[0] = true;
    need[1] = c->res_need[0];
    need[2] = c->res_need[1];
  }
}

static unsigned list_grid(i64 total, unsigned cap) {
  unsigned g = cdiv(total, 256);
  return g > cap ? cap : (g < 1 ? 1 : g);
}

// Grid of a list-driven level.  The kernels grid-stride over whatever the list holds, so the grid
// only has to be big enough to be fast: when the last statistics pass counted the resident states
// above each level, launch about twice that many threads instead of the worst case (the K = 8
// kernel needs 256 VGPRs + scratch per wave; an oversized, mostly idle grid cost 20-70 us).
static unsigned level_grid(const evoamd_ctx *c, const LevelHints &lv, int level, i64 total, unsigned cap, unsigned per_block) {
  unsigned g = list_grid(total, cap);
  const int tag = lv.known_tag;
  if (!c->need_known || tag == 2) return g;
  // candidates / final K^n can exceed a level if a resident state exceeds the level below
  const int src = (tag == 0) ? level : (level > 0 ? level - 1 : 0);
  double expect = lv.scale * c->res_cnt[src] * ((tag == 0) ? 1.0 : 1.0 + (double)c->Cmax / (double)c->S);
  if (tag != 0 && level == 0) expect = (double)total;  // unknown: children of k = 2 parents
  unsigned want = (unsigned)(2.0 * expect / per_block) + 4;
  return want < g ? want : g;
}

// A few thousand states above 4 active latents are served fastest by the wavefront-per-state
// kernel (64 lanes share one k x k system: short latency, 53 vs 100 us at 2.5k states), a large
// population by the K=8 register kernel (one state per thread: 244 us vs 15 ms at 640k states).
static bool use_k8_kernel(const evoamd_ctx *c, const LevelHints &lv) {
  const int tag = lv.known_tag;
  if (c->k8_mode >= 0) return c->k8_mode != 0;
  if (!c->need_known || tag == 2) return true;
  const double expect = c->res_cnt[tag == 0 ? 1 : 0] * (tag == 0 ? 1.0 : (double)c->Cmax / (double)c->S) +
                        (tag == 0 ? 0.0 : c->res_cnt[1]);
  return expect > 8192.0;
}

// Few enough states above 4 active latents (known from the last statistics pass) that the two wavefront levels
// (k <= 8, then k <= KCAP) are better served by one launch at full capacity.
static bool few_dense_states(const evoamd_ctx *c, const LevelHints &lv) {
  const int tag = lv.known_tag;
  if (!c->need_known || tag == 2) return false;
  const double expect = lv.scale * (tag == 0 ? c->res_cnt[1] : c->res_cnt[1] + c->res_cnt[0] * (double)c->Cmax / (double)c->S);
  return expect <= 1024.0;
}

// Few enough states above FOUR active latents that the 5..8 level is not worth a launch of its own (a dependent launch
// costs 10-20 us however little it does -- the c2 shape: 19 such states, three passes per iteration): the pivoting
// wavefront kernel, which runs behind the quad levels anyway, then serves that list as well, at full LDS capacity.
// K^n is close to stationary from one iteration to the next, so the candidates and the final K^n are expected to hold
// about as many such states as the census of the last statistics pass found (x 4 for slack); a wrong guess is only slower.
static bool few_above4(const evoamd_ctx *c, const LevelHints &lv) {
  if (!c->merge_small || !c->need_known || lv.known_tag == 2) return false;
  const double expect = lv.scale * c->res_cnt[1] * (1.0 + 4.0 * (double)c->Cmax / (double)std::max(1, c->S));
  return expect <= 256.0;
}

static int zero_lists(evoamd_ctx *c) {
  if (!c->lists_clean) {
    if (c->pending_skip)  // no clearing kernel ran since the last chain: check its skipped levels here
      check_lists_kernel<<<1, 256, 0, c->stream>>>(c->list_n, 4 * LIST_SHARDS, c->pending_skip, c->err);
    else
      HIP_TRY(hipMemsetAsync(c->list_n, 0, 4 * LIST_SHARDS * sizeof(int), c->stream));
  }
  on_lists_claimed(c);  // the chain about to be launched appends to them
  return 0;
}

static int skip_mask(const bool need[3]) { return (need[0] ? 0 : 1) | (need[1] ? 0 : 2) | (need[2] ? 0 : 4); }

// Census mode (kernels_sssc_quad.hpp): ES3C on complete data with digests -- the resident states above two active latents
// come from lists built once per K^n instead of being appended by the main kernels.
static bool census_mode(const evoamd_ctx *c) {
  return c->model == EVOAMD_MODEL_SSSC && c->clist && c->clist_n && c->ovf_rec && c->use_digest && c->dig && !c->mask_infr;
}

static int ensure_census(evoamd_ctx *c) {
  if (c->census_gen == c->kn_gen) return 0;
  const i64 total = c->N * (i64)c->S;
  // a level that no pass over the OLD census launched must have had an empty list; then fresh counters
  // (evoamd_vary_kn's kernel has done both on its way when it is what changed K^n)
  if (!c->clist_clean) check_lists_kernel<<<1, 256, 0, c->stream>>>(c->clist_n, 4 * LIST_SHARDS, c->census_skip, c->err);
  on_census_claimed(c);
  unsigned grid = cdiv(total, CENSUS_T * CENSUS_PPT);
  if (grid > (unsigned)(8 * c->n_cu)) grid = (unsigned)(8 * c->n_cu);
  SpanGuard g(c, KID_MISC);
  census_kernel<<<grid, CENSUS_T, 0, c->stream>>>(c->dig, total, c->clist, (i64)c->clist_words(), c->clist_n, (int)list_cap(total), c->err);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "census");
  if (c->debug_poison_list) {  // test hook: entry 0 of shard 0 of the 3..4 list becomes an out-of-range (n, state) pair
    c->debug_poison_list = 0;
    const int bad[1] = {0x7FFFFFF0}, one[1] = {1};
    HIP_TRY(hipMemcpyAsync(c->clist, bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->clist_n, one, sizeof(int), hipMemcpyHostToDevice, c->stream));  // (at least that one entry)
    HIP_TRY(hipStreamSynchronize(c->stream));
    on_census_poisoned(c);
    return 0;
  }
  made_census(c);
  return 0;
}

// grid of a quad level (16 states per wave, 64 per workgroup) from the expected number of listed states
static unsigned quad_grid(const evoamd_ctx *c, const LevelHints &lv, int level, i64 total, unsigned cap) {
  return level_grid(c, lv, level, total * 4, cap, 64);
}

// A producer kernel that appends to the pair bins owns region (bin, blockIdx.x) of every bin and counter
// gcnt[bin * nwg + blockIdx.x]: its grid must not exceed pb.nwg (the kernels grid-stride, so a smaller grid is correct).
static unsigned pb_clamp(const PairBins &pb, unsigned grid) {
  return pb.ent && grid > (unsigned)pb.nwg ? (unsigned)pb.nwg : grid;
}
#define PB_GRID_CHECK(pb, grid) \
  REQUIRE(!(pb).ent || (i64)(grid) <= (i64)(pb).nwg, "pair bins: producer grid exceeds the regions per bin (pb.nwg)")

// The kernels that walk a state word by word are instantiated for HW = 1, 2, 4, 8, 16 words and, as 0, with a runtime
// loop for any other count: calls f with the runtime hw as a compile-time constant (std::integral_constant) of that set.
template <class F>
static void with_hw(int hw, F &&f) {
  switch (hw) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

// The one S -> states-per-lane map (S <= 64 x VK_MAX_S_PER_LANE) of the selection, randflip and fused kernels, and the
// Cmax -> candidates-per-lane map of the selection kernel: f gets the value as a compile-time constant.
template <typename F>
static void with_spl(int S, F &&f) {
  if (S <= 64) f(std::integral_constant<int, 1>{});
  else if (S <= 128) f(std::integral_constant<int, 2>{});
  else if (S <= 256) f(std::integral_constant<int, 4>{});
  else if (S <= 512) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}
template <typename F>
static void with_cpl(int Cmax, F &&f) {
  if (Cmax <= 64) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 4>{});
}

// The on-the-fly lists 1..3 of a pass as the kernels append to them (o) and read them (i), the census lists of the resident
// K^n (3..4 / 5..8 / > 8 latents), a list that is always empty (nobody appends to the fourth row of the census counters),
// and "no list".  `cap` is the shard stride: what appended with one capacity is read with the same.
struct Es3cLists {
  ListOut o1, o2, o3;
  ListIn i1, i2, i3;
  ListIn cA, cB, cC;
  ListIn empty;
  ListOut none_out;
  ListIn none_in;
};

static Es3cLists es3c_lists(const evoamd_ctx *c, int cap) {
  Es3cLists ls = {};
  ls.o1 = {c->list1, c->list_n + 0 * LIST_SHARDS, cap};
  ls.o2 = {c->list2, c->list_n + 1 * LIST_SHARDS, cap};
  ls.o3 = {c->list3, c->list_n + 2 * LIST_SHARDS, cap};
  ls.i1 = {ls.o1.items, ls.o1.counts, cap};
  ls.i2 = {ls.o2.items, ls.o2.counts, cap};
  ls.i3 = {ls.o3.items, ls.o3.counts, cap};
  if (c->clist && c->clist_n) {
    ls.cA = {c->clist, c->clist_n, cap};
    ls.cB = {c->clist + c->clist_words(), c->clist_n + LIST_SHARDS, cap};
    ls.cC = {c->clist + 2 * c->clist_words(), c->clist_n + 2 * LIST_SHARDS, cap};
    ls.empty = {c->clist, c->clist_n + 3 * LIST_SHARDS, 0};
  }
  return ls;
}

// ---- the wavefront levels behind the quads of a pass over the census lists, the same launches for the lpj pass (MODE 0,
// the pass's TAG) and the statistics pass (MODE 1): resident states above eight latents + what the quads passed on (list 3).
// Returns the on-the-fly lists it served (bit k - 1 = list k).
template <int MODE, int TAG>
static int census_wavefront_levels(evoamd_ctx *c, const SsscArgs &a, const Es3cLists &ls, const bool need[3], bool few4,
                                   const LevelHints &lv, i64 total) {
  if (few4) {
    // ONE wavefront launch at full capacity: the 5..8 list, the states above eight, what the 3..4 level passed on
    // (nobody appends to list 2)
    sssc_big_kernel<MODE, TAG><<<std::max(64u, level_grid(c, lv, 1, total * 256, 1024, 1)), 64, big_lds(SSSC_KCAP), c->stream>>>(
        a, need[1] ? ls.cB : ls.empty, ls.none_out, SSSC_KCAP, need[2] ? ls.cC : ls.empty, ls.i3);
    return 4;
  }
  // the pivoting wavefront kernel: resident states above eight latents, then what the quads passed on -- sized for
  // 16 latents (6.8 KB of LDS per state: ~20 workgroups per CU; at the full 64 it is 98 KB, ONE per CU, and a dense
  // K^n(0) with 40 % of its states above eight latents took 0.5 s in it), the few states beyond go on to list 2
  sssc_big_kernel<MODE, TAG><<<std::max(256u, level_grid(c, lv, 2, total * 256, 8192, 1)), 64, big_lds(16), c->stream>>>(
      a, need[2] ? ls.cC : ls.empty, ls.o2, 16, ls.i3);
  if (!need[2]) return 4;  // nobody serves list 2: it must be found empty when the counters are cleared
  sssc_big_kernel<MODE, TAG><<<level_grid(c, lv, 2, total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
      a, ls.i2, ls.none_out, SSSC_KCAP);
  return 2 | 4;
}

#define MAIN_LPJ_LDS_MAX (48 * 1024)  // three 512-thread workgroups (3072 pairs) per CU at the limit

// LDS of the table-driven main kernel with the B rows of its workgroup's datapoints staged (1024 pairs per workgroup)
static size_t main_lpj_lds(int C, int H) {
  return ((size_t)(1024 / C + 2) * H + (H <= 512 ? (size_t)4 * H : 0)) * sizeof(double);
}

// ES3C kappa route (option "stats_kappa"): what the lpj passes and the statistics pass both need -- the record buffers
// (allocated by evoamd_configure where H and the options allowed it), census lists, digests, complete data, f64, even H
static bool kappa_shape_ok(const evoamd_ctx *c) {
  return kappa_wanted(c) && c->kap && c->cand_kap && census_mode(c) && (c->H % 2) == 0 && !c->sssc_prec32;
}

enum LpjRoute {
  LPJ_MASKED,  // incomplete data: the wavefront kernel for every pair
  LPJ_CENSUS,  // pass over the resident K^n with census lists: the main kernel appends nothing, the levels read the lists
  LPJ_CHAINS,  // on-the-fly lists, quad levels (option "census_lists" = 1: candidate batches, shared / transient sets)
  LPJ_ROUND2   // on-the-fly lists, register-kernel levels (option "census_lists" = 0)
};
enum LpjMain {
  LPJ_MAIN_NONE,      // levels only
  LPJ_MAIN_CENSUS,    // staged B rows, appends nothing
  LPJ_MAIN_STAGED,    // staged B rows, appends to list 1
  LPJ_MAIN_UNSTAGED,  // the same table-driven kernel with the B values gathered from global memory
  LPJ_MAIN_SMALL      // K = 2 register kernel
};

// What an ES3C lpj pass decides before it enqueues anything (lpj_plan); the stages only read it.
struct LpjPlan {
  LpjRoute route;
  LevelHints lv;
  int kid_main;
  i64 total;
  int cap;
  Es3cLists ls;
  bool need[3];  // overflow levels the batch needs (levels_for)
  bool any;      // ... and whether any runs
  LpjMain main;
  int rows_cap, stage_dg;
  size_t lds;
  unsigned grid;
  bool few4;       // census / chains: the wavefront launch serves the 5..8 list too (few_above4)
  bool k8;         // round 2: K = 8 register kernel (use_k8_kernel)
  bool few_dense;  // round 2: one wavefront launch for lists 2 and 3 (few_dense_states)
  bool kappa;      // the table-driven main kernel leaves the kappa records of its states (K^n: c->kap, candidates: c->cand_kap)
};

// Fills the plan from the context as it is at entry.  Enqueues nothing.  `tag` (Batch::tag) names the kernel
// instantiations of the pass in a trace; what is known about its states is in `lv`.
static void lpj_plan(const evoamd_ctx *c, const SsscArgs &a, int tag, const LevelHints &lv, int kid_main, LpjPlan &p) {
  p = LpjPlan{};
  p.lv = lv;
  p.kid_main = kid_main;
  p.total = a.N * (i64)a.C;
  p.cap = (int)list_cap(p.total);
  p.ls = es3c_lists(c, p.cap);
  levels_for(c, lv, p.need);
  p.any = p.need[0] || p.need[1] || p.need[2];
  const bool tables = !a.shared && (a.H % 2) == 0;  // the table-driven main kernel applies
  const bool staged = tables && main_lpj_lds(a.C, a.H) <= MAIN_LPJ_LDS_MAX;
  if (a.mask)
    p.route = LPJ_MASKED;
  else if (tag == 0 && a.states == c->states && census_mode(c) && staged)
    p.route = LPJ_CENSUS;
  else
    p.route = c->census_opt ? LPJ_CHAINS : LPJ_ROUND2;
  // 512-thread workgroups: measured 13.8-17.5 us without overflow and 20.0 us at 8 % overflow on
  // the c2 shape (256: 13.0 / 24.3 us, 1024: 16.3 / 20.5 us).  The B rows of the workgroup's
  // datapoints (and the per-latent table while it is small) are staged in LDS when they fit.
  // two pairs per thread: 1024 pairs per workgroup
  p.stage_dg = a.H <= 512;
  p.grid = cdiv(p.total, 1024);
  if (staged) {
    p.main = p.route == LPJ_CENSUS ? (lv.levels_only ? LPJ_MAIN_NONE : LPJ_MAIN_CENSUS) : LPJ_MAIN_STAGED;
    p.rows_cap = 1024 / a.C + 2;
    p.lds = main_lpj_lds(a.C, a.H);
  } else if (tables && a.dig && c->main_unstaged) {
    // the rows of the workgroup's datapoints do not fit the LDS (candidate batches: 1024 / Cmax datapoints per workgroup)
    p.main = LPJ_MAIN_UNSTAGED;
    p.lds = (p.stage_dg ? (size_t)4 * a.H : 0) * sizeof(double);
  } else {
    p.main = LPJ_MAIN_SMALL;
    p.grid = cdiv(p.total, 512);
  }
  // kappa records for the statistics pass (option "stats_kappa"): the pass over K^n and the resident candidate batch,
  // on any form of the table-driven main kernel (it evaluates every state with at most two latents in all of them)
  p.kappa = kappa_shape_ok(c) && !lv.levels_only &&
            (p.main == LPJ_MAIN_CENSUS || p.main == LPJ_MAIN_STAGED || p.main == LPJ_MAIN_UNSTAGED) &&
            ((tag == 0 && a.states == c->states && a.C == c->S) || (tag == 1 && a.states == c->cand && a.C == c->Cmax));
  p.few4 = p.route != LPJ_ROUND2 && few_above4(c, lv);
  p.k8 = p.route == LPJ_ROUND2 && use_k8_kernel(c, lv);
  p.few_dense = p.route == LPJ_ROUND2 && few_dense_states(c, lv);
}

// ---- incomplete data: G_A belongs to the datapoint, so no tables and no Gram gathers: the wavefront-per-state kernel
// forms W_obs^T W_obs for every pair (k <= 8 first, the rest via list 3)
static int lpj_sssc_masked(evoamd_ctx *c, const SsscArgs &a, const LpjPlan &p) {
  SpanGuard g(c, p.kid_main);
  const int gridm = (int)std::min<i64>(p.total, 65536);
  sssc_big_kernel<0><<<gridm, 64, big_lds(8), c->stream>>>(a, p.ls.none_in, p.ls.o3, 8);
  sssc_big_kernel<0><<<1024, 64, big_lds(SSSC_KCAP), c->stream>>>(a, p.ls.i3, p.ls.none_out, SSSC_KCAP);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the main kernel: every state with at most two active latents, the rest appended to list 1 (not in census form)
template <int TAG>
static int lpj_sssc_main(evoamd_ctx *c, const SsscArgs &a, const LpjPlan &p) {
  if (p.main == LPJ_MAIN_NONE) return 0;
  SpanGuard g(c, p.kid_main);
  if (p.main == LPJ_MAIN_SMALL)
    sssc_small_kernel<2, 0, TAG, 512><<<p.grid, 512, 0, c->stream>>>(a, p.ls.none_in, p.ls.o1, PairBins{});
  else
    with_hw(a.HW, [&](auto hw) {
      constexpr int HWT = decltype(hw)::value;
      if (p.main == LPJ_MAIN_CENSUS)
        sssc_main_lpj_kernel<TAG, 512, HWT, 2, false><<<p.grid, 512, p.lds, c->stream>>>(a, p.ls.none_out, p.rows_cap, p.stage_dg);
      else if (p.main == LPJ_MAIN_STAGED)
        sssc_main_lpj_kernel<TAG, 512, HWT, 2><<<p.grid, 512, p.lds, c->stream>>>(a, p.ls.o1, p.rows_cap, p.stage_dg);
      else
        sssc_main_lpj_kernel<TAG, 512, HWT, 2, true, false><<<p.grid, 512, p.lds, c->stream>>>(a, p.ls.o1, 0, p.stage_dg);
    });
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, p.main == LPJ_MAIN_CENSUS ? "sssc lpj main (census)" : "sssc lpj main");
  return 0;
}

// ---- the levels of a pass over the census lists: quads on the 3..4 and 5..8 lists, then the wavefront levels
// (the levels carry the pass's TAG in their names, so a kernel trace separates the pass over K^n from the candidate batch
// level by level)
template <int TAG>
static int lpj_sssc_census_levels(evoamd_ctx *c, const SsscArgs &a, const LpjPlan &p, int &served) {
  const Es3cLists &ls = p.ls;
  SpanGuard g(c, KID_LPJ_OVF);
  if (p.need[0]) {
    SpanGuard gl(c, KID_LPJ_K34);
    sssc_quad_kernel<1, 0, TAG><<<quad_grid(c, p.lv, 0, p.total, 2048), 256, 0, c->stream>>>(a, ls.cA, ls.none_out, ls.o3, PairBins{}, nullptr);
  }
  DBG_SYNC(c, "sssc lpj quad level 3..4");
  if (p.need[1] && !p.few4) {
    SpanGuard gl(c, KID_LPJ_K58);
    sssc_quad_kernel<2, 0, TAG><<<quad_grid(c, p.lv, 1, p.total, 2048), 256, 0, c->stream>>>(a, ls.cB, ls.none_out, ls.o3, PairBins{}, nullptr);
  }
  DBG_SYNC(c, "sssc lpj quad level 5..8");
  SpanGuard gl(c, KID_LPJ_K9P);
  served = census_wavefront_levels<0, TAG>(c, a, ls, p.need, p.few4, p.lv, p.total);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, p.few4 ? "sssc lpj census levels (merged)" : "sssc lpj census levels");
  return 0;
}

// ---- the levels of an on-the-fly chain: list 1 -> 3..4 latents -> list 2 -> 5..8 latents (four-lanes-per-state kernel)
// -> list 3 = the pivoting wavefront kernel, which also takes the states the quads pass on and therefore always runs
// behind them
template <int TAG>
static int lpj_sssc_chain_levels(evoamd_ctx *c, const SsscArgs &a, const LpjPlan &p, int &served) {
  const Es3cLists &ls = p.ls;
  SpanGuard g(c, KID_LPJ_OVF);
  // (3..4 latents of a chain: the quad kernel too since round 4 -- the K = 4 thread-per-state register kernel was faster
  // on the ~400k listed candidates of the north-star shape (58 against 77 us), but it eliminates with row exchanges, so a
  // candidate's lpj changed in the last bits when it became a resident state; now every state with 3..4 latents has ONE
  // arithmetic, the one the fused per-datapoint E-step (kernels_fused.hpp) uses as well)
  if (p.need[0])
    sssc_quad_kernel<1, 0, TAG><<<quad_grid(c, p.lv, 0, p.total, 2048), 256, 0, c->stream>>>(a, ls.i1, ls.o2, ls.o3, PairBins{}, nullptr);
  DBG_SYNC(c, "sssc lpj chain 3..4");
  if (p.few4) {
    // (few states above four latents: the wavefront launch serves list 2 as well -- one launch less)
    sssc_big_kernel<0, TAG><<<std::max(64u, level_grid(c, p.lv, 1, p.total * 256, 1024, 1)), 64, big_lds(SSSC_KCAP), c->stream>>>(
        a, ls.i2, ls.none_out, SSSC_KCAP, ls.i3);
    served = 2 | 4;
  } else {
    if (p.need[1])
      sssc_quad_kernel<2, 0, TAG><<<quad_grid(c, p.lv, 1, p.total, 2048), 256, 0, c->stream>>>(a, ls.i2, ls.o3, ls.o3, PairBins{}, nullptr);
    DBG_SYNC(c, "sssc lpj chain 5..8");
    sssc_big_kernel<0, TAG><<<level_grid(c, p.lv, 2, p.total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
        a, ls.i3, ls.none_out, SSSC_KCAP);
    served = 4;
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, p.few4 ? "sssc lpj chain wavefront level (merged)" : "sssc lpj chain wavefront level");
  return 0;
}

// ---- the round-2 levels: list 1 -> K = 4 -> list 2 -> K = 8 / wavefront -> list 3 -> wavefront (stage for stage the
// ladder of stats_sssc_chain_levels, which adds pair bins, in-kernel column sums and its own K = 8 rule)
template <int TAG>
static int lpj_sssc_round2_levels(evoamd_ctx *c, const SsscArgs &a, const LpjPlan &p, int &served) {
  const Es3cLists &ls = p.ls;
  SpanGuard g(c, KID_LPJ_OVF);
  if (p.need[0])
    sssc_small_kernel<4, 0, TAG, 256><<<level_grid(c, p.lv, 0, p.total, 1024, 256), 256, 0, c->stream>>>(a, ls.i1, ls.o2, PairBins{}, ls.o3);
  DBG_SYNC(c, "sssc lpj K=4 level");
  bool merged23 = false;
  if (p.k8) {
    if (p.need[1])
      sssc_small_kernel<8, 0, TAG, 256><<<level_grid(c, p.lv, 1, p.total, 256, 256), 256, 0, c->stream>>>(a, ls.i2, ls.o3, PairBins{}, ls.o3);
  } else if (p.need[1] && p.few_dense) {
    // a handful of states above 4 active latents: ONE launch of the wavefront kernel at full capacity serves list 2
    // (a launch costs ~8 us however little it does; the k <= 8 sizing only pays for thousands of states)
    sssc_big_kernel<0, TAG><<<level_grid(c, p.lv, 1, p.total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
        a, ls.i2, ls.none_out, SSSC_KCAP, ls.i3);  // (list 3: what the K = 4 level passed on in exact mode)
    merged23 = true;
  } else if (p.need[1]) {
    // a few thousand states above 4 active latents: the wavefront-per-state kernel, sized for k <= 8
    // (1.9 KiB of LDS, many workgroups per CU); anything denser moves on to list 3
    sssc_big_kernel<0, TAG><<<level_grid(c, p.lv, 1, p.total * 256, 4096, 1), 64, big_lds(8), c->stream>>>(a, ls.i2, ls.o3, 8);
  }
  DBG_SYNC(c, "sssc lpj K=8 level");
  // (with the screen on, list 3 is served whenever a level ran: in exact mode the register kernels pass their states on)
  if ((p.need[2] || c->sing_screen) && !merged23)
    sssc_big_kernel<0, TAG><<<level_grid(c, p.lv, 2, p.total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
        a, ls.i3, ls.none_out, SSSC_KCAP);
  served = (merged23 || p.need[2] || c->sing_screen) ? 4 : 0;
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "sssc lpj wavefront level");
  return 0;
}

// ES3C lpj of a batch.  The main kernel walks the pairs in natural (coalesced) order and evaluates every state with at
// most two active latents; the states above come from lists -- the census of the resident K^n, or lists the main kernel
// and the levels append to on the fly -- and each level only sees what the previous one could not hold, so waves stay
// homogeneous in k.
//
// A level that is not launched must find its input list empty: the pass leaves in c->pending_skip (on-the-fly lists 1..3 =
// bits 1, 2, 4) and c->census_skip (census lists) what the kernel that clears the counters next has to check
// (check_lists_kernel, census_lists_kernel, tail_kernel).  With skip = skip_mask(need), `levels` = any of need[]:
//
//   route    levels  pending_skip                                                          census_skip
//   masked   -       unchanged                                                             unchanged
//   census   no      unchanged                                                             |= skip (= 7)
//   census   yes     |= 2 unless !few4 && need[2] (the 16-latent launch feeds list 2,      |= skip
//                    only the full-capacity launch behind it serves it)
//   chains   no      |= skip (= 7)                                                         unchanged
//   chains   yes     (|= skip) & ~4, with few4 & ~(2 | 4): the merged launch serves both   unchanged
//   round 2  no      |= skip (= 7)                                                         unchanged
//   round 2  yes     (|= skip), & ~4 if list 3 was served: need[2] || sing_screen ||       unchanged
//                    (!k8 && need[1] && few_dense)
//
// (zero_lists has checked and cleared what the chain before left, so pending_skip is 0 when the table is applied.)
template <int TAG>
static int launch_sssc_lpj(evoamd_ctx *c, const SsscArgs &a_in, int kid_main, const LevelHints &lv) {
  TRY(zero_lists(c));
  LpjPlan p;
  lpj_plan(c, a_in, TAG, lv, kid_main, p);
  SsscArgs a = a_in;
  if (p.kappa) a.kap_out = TAG == 0 ? c->kap.get() : c->cand_kap.get();
  if (TAG == 0 && a.states == c->states) made_kappa(c, p.kappa);
  if (TAG == 1 && a.states == c->cand) made_cand_kappa(c, p.kappa);
  if (p.route == LPJ_MASKED) return lpj_sssc_masked(c, a, p);
  if (p.route == LPJ_CENSUS) TRY(ensure_census(c));
  TRY(lpj_sssc_main<TAG>(c, a, p));
  int served = 0;  // on-the-fly lists the levels read to the end (bit k - 1 = list k)
  if (p.any)
    TRY(p.route == LPJ_CENSUS   ? lpj_sssc_census_levels<TAG>(c, a, p, served)
        : p.route == LPJ_CHAINS ? lpj_sssc_chain_levels<TAG>(c, a, p, served)
                                : lpj_sssc_round2_levels<TAG>(c, a, p, served));
  on_levels_skipped(c, p.route == LPJ_CENSUS, skip_mask(p.need), served, p.any);
  return 0;
}

static int launch_lpj(evoamd_ctx *c, const Batch &b, const LevelHints &lv) {
  if (c->model == EVOAMD_MODEL_BSC) return launch_bsc_lpj(c, b);
  SsscArgs a = sssc_args(c, b);
  if (b.tag == 0) return launch_sssc_lpj<0>(c, a, b.kid, lv);
  if (b.tag == 1) return launch_sssc_lpj<1>(c, a, b.kid, lv);
  return launch_sssc_lpj<2>(c, a, b.kid, lv);
}

static int check_err(evoamd_ctx *c) {
  int *e = c->h_err;
  HIP_TRY(hipMemcpyAsync(e, c->err, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (e[0]) {
    HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int), c->stream));
    if (e[0] & 4) return fail(EVOAMD_E_INVALID, "internal: an ES3C overflow level was skipped although its list was not empty");
    if (e[0] & EVO_ERR_LIST_FULL) return fail(EVOAMD_E_INVALID, "internal: an ES3C overflow list was full, states were dropped");
    if (e[0] & EVO_ERR_BAD_ENTRY) return fail(EVOAMD_E_INVALID, "internal: an ES3C list entry or latent index read back from LDS was out of range");
    if (e[0] & 1) return fail(EVOAMD_E_KLIMIT, "ES3C: a state has more than %d active latents", SSSC_KCAP);
    return fail(EVOAMD_E_SINGULAR, "ES3C: exactly singular k x k system (the reference takes pinv here)");
  }
  return 0;
}

static int lpj_resident_launch(evoamd_ctx *c, double *out, const LevelHints &lv) {
  TRY(ensure_B(c));
  on_lpj_overwritten(c);
  if (c->S_perm) {
    allzero_lpj_kernel<<<cdiv(c->N, 256), 256, 0, c->stream>>>(c->yy, c->N, c->dpar, c->model == EVOAMD_MODEL_SSSC,
                                                               out, c->L, c->flags + 2 * c->N, c->err);
    HIP_TRY(hipGetLastError());
  }
  Batch b = {c->states, nullptr, c->Y, c->Bm, c->yy, c->N, c->S, 0, out, c->L, c->S_perm, c->flags, KID_LPJ_RES, 0};
  b.mask = c->mask_infr;
  SpanGuard pass(c, KID_LPJ_PASS);  // main kernel + every overflow level: everything that produces the N x S lpj
  return launch_lpj(c, b, lv);  // stream-ordered; device-side errors surface at the next host-returning call
}

// ---- E-step stage: lpj of the resident K^n
static int estep_resident_pass(evoamd_ctx *c) {
  if (c->prefetch_gen == c->gen) {  // evoamd_mstep_device already enqueued exactly this pass
    drop_prefetch(c);
    std::swap(c->lpj, c->lpj_alt);
    made_lpj_rows(c);
    return 0;
  }
  TRY(lpj_resident_launch(c, c->lpj, batch_hints(c, 0)));
  made_lpj_rows(c);
  return 0;
}

// the argument checks the E-step entry points share (evoamd_evolve_states has wider rules of its own for the rest)
static int estep_check_ready(const evoamd_ctx *c) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "configure, upload_data and set_params first");
  return 0;
}
static int estep_check_parents(const evoamd_ctx *c, int n_parents) {
  REQUIRE(n_parents >= 1 && n_parents <= c->S && n_parents <= 64, "n_parents must be in [1, min(S, 64)]");
  return 0;
}
static int estep_check_randflip(const evoamd_ctx *c, int n_parents, int n_children) {
  TRY(estep_check_ready(c));
  TRY(estep_check_parents(c, n_parents));
  REQUIRE(n_children >= 1 && n_children <= EV_MAX_CHILDREN && n_children <= c->H, "n_children must be in [1, min(8, H)]");
  REQUIRE(n_parents * n_children <= c->Cmax, "n_parents * n_children exceeds the configured Cmax");
  return 0;
}
static int estep_check_mprime(const evoamd_ctx *c, int Mprime) {
  REQUIRE(Mprime >= 1 && Mprime <= c->S, "Mprime must be in [1, S]");
  return 0;
}

extern "C" int evoamd_lpj_resident(evoamd_ctx *c) {
  TRY(estep_check_ready(c));
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  return estep_resident_pass(c);
}

static int eval_candidates(evoamd_ctx *c) {
  TRY(ensure_B(c));
  Batch b = {c->cand, c->cand_counts, c->Y, c->Bm, c->yy, c->N, c->Cmax, 0, c->cand_lpj, c->Cmax, 0,
             c->flags + c->N, KID_LPJ_CAND, 1};
  b.mask = c->mask_infr;
  return launch_lpj(c, b, batch_hints(c, b.tag));
}

extern "C" int evoamd_lpj_candidates(evoamd_ctx *c, const uint8_t *cand_bool, const int32_t *counts, int Cmax,
                                     double *lpj_out) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "configure, upload_data and set_params first");
  REQUIRE(cand_bool && counts, "NULL candidate batch");
  REQUIRE(Cmax == c->Cmax, "Cmax differs from the configured value");
  HIP_TRY(hipSetDevice(c->device));
  TRY(pack_to_device(c, cand_bool, c->N * (i64)Cmax, c->cand));
  HIP_TRY(hipMemcpyAsync(c->cand_counts, counts, (size_t)c->N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  on_cand_installed(c, /*near_parents=*/false);
  TRY(eval_candidates(c));
  if (lpj_out)
    HIP_TRY(hipMemcpyAsync(lpj_out, c->cand_lpj, (size_t)c->N * Cmax * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
  made_cand_lpj(c);
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_set_candidates(evoamd_ctx *c, const uint8_t *cand_bool, const int32_t *counts, int Cmax,
                                     const double *lpj) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(cand_bool && counts && lpj, "NULL argument");
  REQUIRE(Cmax == c->Cmax, "Cmax differs from the configured value");
  HIP_TRY(hipSetDevice(c->device));
  TRY(pack_to_device(c, cand_bool, c->N * (i64)Cmax, c->cand));
  HIP_TRY(hipMemcpyAsync(c->cand_counts, counts, (size_t)c->N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->cand_lpj, lpj, (size_t)c->N * Cmax * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_cand_installed(c, /*near_parents=*/false);
  made_cand_lpj(c);
  return 0;
}

extern "C" int evoamd_lpj_shared(evoamd_ctx *c, const uint8_t *states_bool, int C, double *lpj_out) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "configure, upload_data and set_params first");
  REQUIRE(states_bool && lpj_out && C > 0, "bad arguments");
  REQUIRE((i64)c->N * C < 2147483647LL, "N * C must fit in int32");
  HIP_TRY(hipSetDevice(c->device));
  TRY(c->tmp_states.ensure(c, (size_t)C * c->HW));
  TRY(c->tmp_lpj.ensure(c, (size_t)c->N * C));
  TRY(ensure_B(c));
  // stage through a private buffer (C*H may exceed the configured staging area)
  DevBuf<uint8_t> st;
  TRY(st.alloc((size_t)C * c->H));
  HIP_TRY(hipMemcpyAsync(st, states_bool, (size_t)C * c->H, hipMemcpyHostToDevice, c->stream));
  pack_states_kernel<<<cdiv((i64)C * c->HW, 256), 256, 0, c->stream>>>(st, c->tmp_states, C, c->H, c->HW);
  if (c->model == EVOAMD_MODEL_SSSC) TRY(ensure_lists(c, (i64)c->N * C));
  Batch b = {c->tmp_states, nullptr, c->Y, c->Bm, c->yy, c->N, C, 1, c->tmp_lpj, C, 0, c->flags + c->N, KID_MISC, 2};
  b.mask = c->mask_infr;
  int r = launch_lpj(c, b, batch_hints(c, b.tag));
  if (!r) {
    hipError_t e = hipMemcpyAsync(lpj_out, c->tmp_lpj, (size_t)c->N * C * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) r = fail(EVOAMD_E_HIP, "lpj_shared copy back: %s", hipGetErrorString(e));
  }
  if (r) return r;
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  return 0;
}

static int lpj_single_impl(evoamd_ctx *c, const double *y, const uint8_t *x_infr, const uint8_t *states_bool, int C,
                           double *lpj_out, int32_t *flags_out) {
  REQUIRE(c && c->configured && c->have_params, "configure and set_params first");
  REQUIRE(y && states_bool && lpj_out && C > 0, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  TRY(c->tmp_states.ensure(c, (size_t)C * c->HW));
  TRY(c->tmp_lpj.ensure(c, (size_t)C + 2));
  TRY(c->tmp_y.ensure(c, (size_t)c->D + c->H + 2));
  TRY(c->stage.ensure(c, (size_t)C * c->H));
  if (c->model == EVOAMD_MODEL_SSSC) TRY(ensure_lists(c, C));
  double *dy = c->tmp_y, *db = c->tmp_y + c->D, *dyy = c->tmp_y + c->D + c->H;
  unsigned *dfl = (unsigned *)(c->tmp_lpj + C);
  HIP_TRY(hipMemcpyAsync(dy, y, (size_t)c->D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  uint8_t *dmask = nullptr;
  if (x_infr) {  // one row of x_infr behind the packed states' staging area
    TRY(c->stage.ensure(c, (size_t)C * c->H + c->D));
    dmask = c->stage + (size_t)C * c->H;
    HIP_TRY(hipMemcpyAsync(dmask, x_infr, (size_t)c->D, hipMemcpyHostToDevice, c->stream));
    mask_apply_kernel<<<cdiv(c->D, 256), 256, 0, c->stream>>>(dy, c->D, dmask, 1, c->D);
    if (c->model == EVOAMD_MODEL_SSSC && !c->mask_infr) {
      // no resident masks: nobody has allocated W^T or kept it current (derive_from_theta transposes only with masks
      // resident), and the wavefront kernel forms W_obs^T W_obs from it
      if (!c->Wt) TRY(c->Wt.alloc((size_t)c->H * c->D));
      transpose_kernel<<<cdiv((i64)c->H * c->D, 256), 256, 0, c->stream>>>(c->W, c->D, c->H, c->Wt);
    }
  }
  HIP_TRY(hipMemcpyAsync(c->stage, states_bool, (size_t)C * c->H, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(dfl, 0, sizeof(unsigned), c->stream));
  pack_states_kernel<<<cdiv((i64)C * c->HW, 256), 256, 0, c->stream>>>(c->stage, c->tmp_states, C, c->H, c->HW);
  row_sqnorm_kernel<<<1, 256, 0, c->stream>>>(dy, c->D, 1, c->D, dyy);
  if (c->model == EVOAMD_MODEL_SSSC) TRY(launch_gemm_nn(c, dy, c->D, c->W, c->H, db, c->H, 1, c->H, c->D));
  Batch b = {c->tmp_states, nullptr, dy, db, dyy, 1, C, 1, c->tmp_lpj, C, 0, dfl, KID_MISC, 2};
  b.mask = dmask;
  TRY(launch_lpj(c, b, batch_hints(c, b.tag)));
  unsigned fl = 0;
  HIP_TRY(hipMemcpyAsync(lpj_out, c->tmp_lpj, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&fl, dfl, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (flags_out) {
    flags_out[0] = (fl & EVO_FLAG_NAN) ? 1 : 0;
    flags_out[1] = (fl & EVO_FLAG_NEGINF) ? 1 : 0;
    flags_out[2] = (fl & (EVO_FLAG_NEGINF | EVO_FLAG_POSINF)) ? 1 : 0;
  }
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  return 0;
}

extern "C" int evoamd_lpj_single(evoamd_ctx *c, const double *y, const uint8_t *states_bool, int C,
                                 double *lpj_out, int32_t *flags_out) {
  return lpj_single_impl(c, y, nullptr, states_bool, C, lpj_out, flags_out);
}

extern "C" int evoamd_lpj_single_masked(evoamd_ctx *c, const double *y, const uint8_t *x_infr,
                                        const uint8_t *states_bool, int C, double *lpj_out, int32_t *flags_out) {
  REQUIRE(x_infr, "x_infr is NULL");
  return lpj_single_impl(c, y, x_infr, states_bool, C, lpj_out, flags_out);
}

// ---------------------------------------------------------------------------------------
// selection
// ---------------------------------------------------------------------------------------
// ---- E-step stage: selection (vary_Kn) over the resident candidate batch
static int estep_select(evoamd_ctx *c, int Mprime, double *sums_out) {
  on_kn_changed(c, KN_BY_SELECTION);
  {
    SpanGuard g(c, KID_VARY_KN);
    int *cl_n = census_mode(c) ? c->clist_n : nullptr;  // the old census dies with the old K^n: checked + cleared on the way
    const i64 zero_n = c->fold_clear ? (i64)(c->ovf_n + c->acc_n) : 0;  // ... and the next statistics pass finds its accumulators zeroed
    if (!c->fold_clear) cl_n = nullptr;
    const bool kap_carry = c->kap_carry && c->kap && c->cand_kap;  // both sides hold current kappa records: they move along
    with_spl(c->S, [&](auto spl) {
      with_cpl(c->Cmax, [&](auto cpl) {
        vary_kn_kernel<decltype(spl)::value, decltype(cpl)::value><<<cdiv(c->N, 4), 256, 0, c->stream>>>(
            c->states, c->lpj, c->cand, c->cand_lpj, c->cand_counts, c->N, c->S, c->S_perm, c->HW, c->Cmax, Mprime, c->rowmax,
            c->rowsum, c->partial, c->list_n, 4 * LIST_SHARDS, c->dig, c->cand_dig, (c->use_digest && c->dig) ? 1 : 0,
            c->pending_skip, c->err, cl_n, 4 * LIST_SHARDS, c->census_skip, c->acc_base, zero_n,
            kap_carry ? c->kap.get() : nullptr, kap_carry ? c->cand_kap.get() : nullptr);
      });
    });
    reduce3_partials_kernel<<<1, R3_THREADS, 0, c->stream>>>(c->partial, cdiv(c->N, 4), c->dpar);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "vary_kn");
    made_selection(c, cl_n != nullptr, zero_n > 0, kap_carry);
  }
  if (sums_out) {
    HIP_TRY(hipMemcpyAsync(sums_out, c->dpar + DP_ECNT0, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return 0;
}

extern "C" int evoamd_vary_kn(evoamd_ctx *c, int Mprime, double *sums_out) {
  REQUIRE(c && c->configured && c->have_cand, "no resident candidate batch (call lpj_candidates / evolve first)");
  TRY(estep_check_mprime(c, Mprime));
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  return estep_select(c, Mprime, sums_out);
}

extern "C" int evoamd_set_estep_counts(evoamd_ctx *c, double sum_nunique, double sum_sub) {
  REQUIRE(c && c->configured, "configure first");
  HIP_TRY(hipSetDevice(c->device));
  double v[2] = {sum_nunique, sum_sub};
  HIP_TRY(hipMemcpyAsync(c->dpar + DP_ECNT0, v, sizeof(v), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- E-step stage: randflip children of the selected parents and their lpj
static int estep_children(evoamd_ctx *c, int n_parents, int n_children, uint64_t seed, int fit_parents) {
  {
    SpanGuard g(c, KID_EVOLVE);
    with_spl(c->S, [&](auto spl) {
      evolve_randflip_kernel<decltype(spl)::value><<<cdiv(c->N, 4), 256, 0, c->stream>>>(
          c->states, c->lpj, c->N, c->S, c->S_perm, c->H - c->bg_unit, c->HW, n_parents, n_children, c->Cmax, seed, fit_parents,
          c->cand, c->cand_counts, c->list_n, c->model == EVOAMD_MODEL_SSSC ? 4 * LIST_SHARDS : 0, c->cand_dig, c->pending_skip,
          c->err);
    });
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "evolve");
    made_clean_lists(c);
    on_cand_installed(c, /*near_parents=*/true);
  }
  TRY(eval_candidates(c));
  made_cand_lpj(c);
  return 0;
}

extern "C" int evoamd_evolve_randflip(evoamd_ctx *c, int n_parents, int n_children, uint64_t seed, int fit_parents) {
  TRY(estep_check_randflip(c, n_parents, n_children));
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  return estep_children(c, n_parents, n_children, seed, fit_parents);
}

// ---------------------------------------------------------------------------------------
// The whole E-step of the device-RNG path in ONE call (sssc.py:510-552 / _models.py:497-538 for every datapoint):
// lpj of K^n, randflip children of n_parents selected parents, their lpj, vary_Kn.  Where the shape allows it (ES3C,
// complete data, digests, S_perm = 0, at most 64 children, H <= 1024) and K^n is sparse enough, ONE fused kernel does it
// per datapoint (kernels_fused.hpp); otherwise the separate passes run -- same results bit for bit.
// ---------------------------------------------------------------------------------------
static bool fused_shape_ok(const evoamd_ctx *c, int n_parents, int n_children) {
  // (the LDS condition is the one under which launch_sssc_lpj<0> serves K^n from the census lists)
  return c->model == EVOAMD_MODEL_SSSC && c->S_perm == 0 && !c->bg_unit && !c->mask_infr && c->use_digest && c->dig && census_mode(c) &&
         c->H <= 1024 && c->H >= 2 && (c->H % 2) == 0 && n_parents * n_children <= 64 && n_parents * n_children <= c->Cmax &&
         c->rowF && c->defer &&
         ((size_t)(1024 / c->S + 2) * c->H + (c->H <= 512 ? (size_t)4 * c->H : 0)) * sizeof(double) <= MAIN_LPJ_LDS_MAX;
}

#define FUSED_LDS_MAX (150 * 1024)  // dynamic LDS of one workgroup of the fused kernel
// Shards below this many resident states: the fused kernel lists the census of the NEW K^n itself (a launch saved); on
// larger ones census_kernel does (its 35-47 us at the north-star shape are less than the ~70 the ballots and reservations
// cost inside the fused kernel).  Read by the launch and by the census "made" event.
static const i64 INKERNEL_CENSUS_BELOW = (i64)4 << 20;

// One launch of the fused kernel.  Two launches of one body: every datapoint with LDS for 16 latents per pivoted child,
// then -- from a list on the device, empty in practice -- the datapoints that met a denser child, one wave per workgroup
// with LDS for SSSC_KCAP latents.
struct FusedStage {
  int W, kc_big, lds_wave_bytes;
  size_t lds;
  unsigned grid;
};
// Every host decision of evoamd_estep.  Filled by estep_plan from the context as it is at entry; enqueues nothing.
struct EstepPlan {
  bool fused = false;            // one fused kernel per datapoint, else the separate passes
  int spl = 1;                   // states per lane (with_spl)
  bool inkernel_census = false;  // fused route: the kernel lists the new K^n
  FusedStage st[2] = {};
};

static int estep_plan(const evoamd_ctx *c, int n_parents, int n_children, EstepPlan &p) {
  p = EstepPlan{};
  with_spl(c->S, [&](auto spl) { p.spl = decltype(spl)::value; });
  // Sparse enough: FAST leaves every datapoint that meets a state above four latents to the low-occupancy FULL launches
  // -- the census of the last statistics pass says how many states there are above four
  p.fused = c->fused_opt != 0 && fused_shape_ok(c, n_parents, n_children);
  if (p.fused && c->fused_opt == 1) p.fused = c->need_known && c->res_cnt[1] <= 0.25 * (double)c->N;
  if (!p.fused) return 0;
  p.inkernel_census = c->N * (i64)c->S < INKERNEL_CENSUS_BELOW;
  const size_t tab = (size_t)4 * c->H * sizeof(double);
  for (int stage = 0; stage < 2; stage++) {
    FusedStage &st = p.st[stage];
    st.W = stage == 0 ? 4 : 1;
    st.kc_big = stage == 0 ? 16 : SSSC_KCAP;
    st.lds_wave_bytes = fused_lds_wave_bytes(p.spl, st.kc_big);
    auto lds_of = [&](int w) { return (stage == 0 ? tab : 0) + (size_t)w * st.lds_wave_bytes; };
    while (stage == 1 && lds_of(1) > FUSED_LDS_MAX && st.kc_big > 16) {  // (S = 1024: the rows leave room for fewer latents)
      st.kc_big -= 4;
      st.lds_wave_bytes = fused_lds_wave_bytes(p.spl, st.kc_big);
    }
    while (st.W > 1 && lds_of(st.W) > FUSED_LDS_MAX) st.W >>= 1;
    st.lds = lds_of(st.W);
    REQUIRE(st.lds <= FUSED_LDS_MAX, "fused E-step: S too large for the LDS rows");
    int per_cu = (int)((160 * 1024) / (st.lds + 256));
    per_cu = std::max(1, std::min(per_cu, 8 / st.W));  // two waves per SIMD (256 registers; four waves with scratch traffic ran the same)
    st.grid = (unsigned)std::min<i64>(cdiv(c->N, st.W), (i64)c->n_cu * per_cu);
  }
  return 0;
}

static int flush_reduce(evoamd_ctx *c);

// ---- fused stage: resident states above two latents -- the list kernels over the census of THIS K^n (built by the last
// fused call or by census_kernel), sixteen states per wave pass; their values land in the lpj row the fused kernel reads
static int estep_fused_levels(evoamd_ctx *c) {
  LevelHints lv = batch_hints(c, 0);
  lv.levels_only = true;
  return lpj_resident_launch(c, c->lpj, lv);
}

// ---- fused stage: the argument block both launches share (the per-launch fields: estep_fused_launch)
static FusedArgs estep_fused_args(evoamd_ctx *c, const EstepPlan &p, int n_parents, int n_children, uint64_t seed, int fit_parents,
                                  int Mprime) {
  Batch b = {c->states, nullptr, c->Y, c->Bm, c->yy, c->N, c->S, 0, c->lpj, c->L, 0, c->flags, KID_LPJ_RES, 0};
  FusedArgs f = {};
  f.a = sssc_args(c, b);
  f.states = c->states, f.dig = c->dig, f.lpj = c->lpj, f.S = c->S;
  f.n_parents = n_parents, f.n_children = n_children, f.fit_parents = fit_parents, f.Mprime = Mprime, f.seed = seed;
  f.rowmax = c->rowmax, f.rowsum = c->rowsum, f.rowF = c->rowF, f.rowcnt = c->rowcnt;
  f.flags_res = c->flags, f.flags_cand = c->flags + c->N;
  f.list_cap = (int)c->N;
  f.cand = c->cand, f.Cmax = c->Cmax;
  if (p.inkernel_census) {
    f.cen_items = c->clist;
    f.cen_n = c->clist_n;
    f.cen_stride = (i64)c->clist_words();
    f.cen_cap = (int)list_cap(c->N * (i64)c->S);
  }
  return f;
}

#ifdef FUSED_PROFILE
static int estep_fused_profile(evoamd_ctx *c) {
  unsigned long long h[8];
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(h, c->fprof, sizeof(h), hipMemcpyDeviceToHost));
  if ((c->fused_calls % 50) == 49) {
    fprintf(stderr, "[fused profile] wave cycles per datapoint:");
    for (int i = 0; i < 8; i++) fprintf(stderr, " p%d %.0f", i, (double)h[i] / (double)c->N / (double)(c->fused_calls + 1));
    fprintf(stderr, "\n");
  }
  return 0;
}
#endif

// ---- fused stage: the deferral counter, the old census's check where the kernel lists the new one, the two launches
static int estep_fused_launch(evoamd_ctx *c, const EstepPlan &p, FusedArgs &f) {
  int *list1 = c->defer, *cnt1 = c->defer + c->N;
  HIP_TRY(hipMemsetAsync(cnt1, 0, sizeof(int), c->stream));
  if (p.inkernel_census) {
    check_lists_kernel<<<1, 256, 0, c->stream>>>(c->clist_n, 4 * LIST_SHARDS, c->census_skip, c->err);
    on_census_claimed(c);  // the fused kernel appends to them
  }
  SpanGuard g(c, KID_ESTEP_FUSED);
  for (int stage = 0; stage < 2; stage++) {
    const FusedStage &st = p.st[stage];
    f.in_items = stage == 0 ? nullptr : list1;
    f.in_count = stage == 0 ? nullptr : cnt1;
    f.out_items = stage == 0 ? list1 : nullptr;
    f.out_count = stage == 0 ? cnt1 : nullptr;
    f.kc_big = st.kc_big;
    f.stage_d1 = stage == 0;
    f.lds_wave_bytes = st.lds_wave_bytes;
    with_spl(c->S, [&](auto spl) {
      if (stage)
        sssc_estep_fused_kernel<decltype(spl)::value, true><<<st.grid, 64 * st.W, st.lds, c->stream>>>(f);
      else
        sssc_estep_fused_kernel<decltype(spl)::value, false><<<st.grid, 64 * st.W, st.lds, c->stream>>>(f);
    });
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, stage == 0 ? "fused E-step" : "fused E-step (listed datapoints, KCAP latents)");
  }
  made_fused_rows(c, /*reduced=*/false);  // summed in front of the first reader (statistics pass: beside the forked contraction)
  return 0;
}

// rowF / rowcnt of the fused E-step -> dpar[DP_FS], dpar[DP_ECNT0 / 1]
static int flush_reduce(evoamd_ctx *c) {
  if (!c->reduce_pending) return 0;
  made_fused_rows(c, /*reduced=*/true);
  fused_reduce3_kernel<<<FR3_BLOCKS, R3_THREADS / FR3_BLOCKS, 0, c->stream>>>(c->rowF, c->rowcnt, c->N, c->dpar, c->fpart,
                                                                              (unsigned *)(c->defer + 2 * (c->N + 1)));
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "fused E-step (reduce)");
  return 0;
}

extern "C" int evoamd_estep(evoamd_ctx *c, int n_parents, int n_children, uint64_t seed, int fit_parents, int Mprime, int *fused_out) {
  TRY(estep_check_randflip(c, n_parents, n_children));
  TRY(estep_check_mprime(c, Mprime));
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  EstepPlan p;
  TRY(estep_plan(c, n_parents, n_children, p));
  if (fused_out) *fused_out = p.fused ? 1 : 0;
  if (!p.fused) {
    c->unfused_calls++;
    on_estep_route(c, /*fused=*/false);
    TRY(estep_resident_pass(c));
    TRY(estep_children(c, n_parents, n_children, seed, fit_parents));
    return estep_select(c, Mprime, nullptr);
  }
  c->fused_calls++;
  drop_prefetch(c);  // a prefetched pass over K^n (if any) is not needed
  on_lpj_overwritten(c);
  TRY(flush_reduce(c));  // (a previous fused E-step whose counters nobody has read yet)
  TRY(ensure_B(c));
  FusedArgs f = estep_fused_args(c, p, n_parents, n_children, seed, fit_parents, Mprime);
#ifdef FUSED_PROFILE
  if (!c->fprof) {
    TRY(c->fprof.alloc(8));
    HIP_TRY(hipMemset(c->fprof, 0, 8 * sizeof(unsigned long long)));
  }
  f.prof = c->fprof;
#endif
  TRY(estep_fused_levels(c));
  TRY(estep_fused_launch(c, p, f));
#ifdef FUSED_PROFILE
  TRY(estep_fused_profile(c));
#endif
  made_fused_estep(c, p.inkernel_census);
  return 0;
}

extern "C" int evoamd_estep_counters(evoamd_ctx *c, int64_t out[4]) {
  REQUIRE(c && c->configured && out, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  out[0] = c->fused_calls;
  out[1] = c->unfused_calls;
  out[2] = out[3] = 0;
  if (c->defer) {
    int h[2] = {0, 0};
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&h[0], c->defer + c->N, sizeof(int), hipMemcpyDeviceToHost));
    out[2] = h[0];
  }
  return 0;
}

// the argument checks of the general operators (evoamd_evolve_states, and evoamd_refine_states where it uses them)
static int estep_check_evolve(const evoamd_ctx *c, int mutation, int n_parents, int n_children, int n_generations,
                              double bitflip_prob) {
  TRY(estep_check_ready(c));
  REQUIRE(mutation >= EV_RANDFLIP && mutation <= EV_CROSS_SPARSEFLIP, "unknown mutation operator");
  REQUIRE_KN(c);
  TRY(estep_check_parents(c, n_parents));
  REQUIRE(n_generations >= 1, "n_generations must be positive");
  const bool crossing = mutation >= EV_CROSS;
  const int per_gen = crossing ? n_parents * (n_parents - 1) : n_parents * n_children;
  REQUIRE(crossing || (n_children >= 1 && n_children <= c->H), "n_children must be in [1, H]");
  REQUIRE(mutation != EV_RANDFLIP || n_children <= EV_MAX_CHILDREN, "randflip: n_children must be <= 8");
  REQUIRE((i64)per_gen * n_generations <= c->Cmax, "children per generation x generations exceeds the configured Cmax");
  REQUIRE(c->S <= EVG_MAX_S && c->Cmax <= EVG_MAX_C, "S <= 1024 and Cmax <= 256");
  const bool sparse = mutation == EV_SPARSEFLIP || mutation == EV_CROSS_SPARSEFLIP;
  REQUIRE(!sparse || bitflip_prob == bitflip_prob, "sparseflip needs bitflip_prob (eas.py:69)");
  REQUIRE(!crossing || c->H >= 2, "crossover needs H >= 2");
  return 0;
}

// ---- E-step stage: children of any operator over any number of generations, and their lpj
static int estep_children_general(evoamd_ctx *c, int mutation, int fit_parents, int n_parents, int n_children,
                                  int n_generations, uint64_t seed, double sparseness, double bitflip_prob) {
  if (!c->cand_raw) {
    TRY(c->cand_raw.alloc((size_t)c->N * c->Cmax * c->HW));
    TRY(c->dupold.alloc((size_t)c->N * EVG_FLAGW));
    TRY(c->gen_start.alloc((size_t)c->N));
  }
  EvolveArgs a = {};
  a.states = c->states;
  a.dig = c->use_digest ? c->dig : nullptr;
  a.lpj = c->lpj;
  a.cand = c->cand;
  a.cand_dig = c->cand_dig;
  a.cand_lpj = c->cand_lpj;
  a.raw = c->cand_raw;
  a.counts = c->cand_counts;
  a.gen_start = c->gen_start;
  a.dupold = c->dupold;
  a.N = c->N;
  a.S = c->S;
  a.S_perm = c->S_perm;
  a.H = c->H - c->bg_unit;  // the operators' domain: without the permanent background unit (eas.py:213-239)
  a.HW = c->HW;
  a.Cmax = c->Cmax;
  a.n_parents = n_parents;
  a.n_children = n_children;
  a.kind = mutation;
  a.fit_parents = fit_parents;
  a.seed = seed;
  a.sparseness = sparseness;
  a.p_bf = bitflip_prob;
  for (int g = 0; g < n_generations; g++) {
    a.gen = g;
    {
      SpanGuard sg(c, KID_EVOLVE);
      evolve_general_kernel<<<(unsigned)c->N, 64, 0, c->stream>>>(a);
      HIP_TRY(hipGetLastError());
      DBG_SYNC(c, "evolve (general)");
    }
    on_cand_installed(c, /*near_parents=*/false);  // children may differ from every resident state in many bits
    TRY(eval_candidates(c));  // the next generation's pool needs these lpj (eas.py:264)
  }
  made_cand_lpj(c);
  return 0;
}

extern "C" int evoamd_evolve_states(evoamd_ctx *c, int mutation, int fit_parents, int n_parents, int n_children,
                                    int n_generations, uint64_t seed, double sparseness, double bitflip_prob) {
  TRY(estep_check_evolve(c, mutation, n_parents, n_children, n_generations, bitflip_prob));
  HIP_TRY(hipSetDevice(c->device));
  return estep_children_general(c, mutation, fit_parents, n_parents, n_children, n_generations, seed, sparseness,
                                bitflip_prob);
}

extern "C" int evoamd_download_candidates(evoamd_ctx *c, uint8_t *cand_bool, int32_t *counts, double *lpj) {
  REQUIRE(c && c->configured && c->have_cand, "no resident candidate batch");
  REQUIRE(cand_bool && counts && lpj, "NULL output");
  HIP_TRY(hipSetDevice(c->device));
  const i64 ns = c->N * (i64)c->Cmax;
  TRY(c->stage.ensure(c, (size_t)ns * c->H));
  unpack_states_kernel<<<cdiv(ns * c->H, 256), 256, 0, c->stream>>>(c->cand, c->stage, ns, c->H, c->HW);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cand_bool, c->stage, (size_t)ns * c->H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(counts, c->cand_counts, (size_t)c->N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(lpj, c->cand_lpj, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// K^n refined at fixed Theta: the E-step stages in a loop (kernels_refine.hpp).  One pass over the resident K^n at
// entry; after that the selection kernel keeps the lpj rows current (it writes the lpj of every state it swaps in), so an
// iteration is children, their lpj, selection and one trace row.  Never the fused kernel: it evaluates K^n itself.
// ---------------------------------------------------------------------------------------
static int refine_trace(evoamd_ctx *c, i64 row, int mode) {
  SpanGuard g(c, KID_MISC);
  refine_trace_kernel<<<1, 64, 0, c->stream>>>(c->dpar, row < 0 ? nullptr : c->refine_trace + 3 * row, mode);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "refine trace");
  return 0;
}

extern "C" int evoamd_refine_states(evoamd_ctx *c, int n_iterations, int mutation, int fit_parents, int n_parents,
                                    int n_children, int n_generations, uint64_t seed0, uint64_t seed_stride,
                                    double sparseness, double bitflip_prob, int Mprime, int check_every, int patience,
                                    double min_sub, double *trace_out, int *n_done_out) {
  const bool fast = mutation == EV_RANDFLIP && n_generations == 1 && n_children <= EV_MAX_CHILDREN;
  if (fast)
    TRY(estep_check_randflip(c, n_parents, n_children));
  else
    TRY(estep_check_evolve(c, mutation, n_parents, n_children, n_generations, bitflip_prob));
  TRY(estep_check_mprime(c, Mprime));
  REQUIRE_KN(c);
  REQUIRE(n_iterations >= 1, "evoamd_refine_states: n_iterations must be positive");
  REQUIRE(patience <= 0 || check_every >= 1, "evoamd_refine_states: check_every must be positive when patience is");
  REQUIRE(trace_out && n_done_out, "evoamd_refine_states: trace_out / n_done_out is NULL");
  HIP_TRY(hipSetDevice(c->device));
  TRY(c->refine_trace.ensure(c, (size_t)3 * n_iterations));
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));
  TRY(refine_trace(c, -1, REFINE_TRACE_ZERO));  // (counts nobody has read yet would end up in row 0)
  int done = 0, copied = 0;
  while (done < n_iterations) {
    const uint64_t seed = seed0 + (uint64_t)done * seed_stride;
    if (fast)
      TRY(estep_children(c, n_parents, n_children, seed, fit_parents));
    else
      TRY(estep_children_general(c, mutation, fit_parents, n_parents, n_children, n_generations, seed, sparseness,
                                 bitflip_prob));
    TRY(estep_select(c, Mprime, nullptr));
    TRY(refine_trace(c, done, REFINE_TRACE_ROW));
    done++;
    if (patience > 0 && (done % check_every == 0 || done == n_iterations)) {  // the chunk's rows: the one wait of the loop
      HIP_TRY(hipMemcpyAsync(trace_out + 3 * copied, c->refine_trace + 3 * copied, (size_t)3 * (done - copied) * sizeof(double),
                             hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      copied = done;
      bool quiet = done >= patience;
      for (int t = done - patience; quiet && t < done; t++) quiet = trace_out[3 * t + 2] / (double)c->N <= min_sub;
      if (quiet) break;
    }
  }
  TRY(refine_trace(c, done - 1, REFINE_TRACE_RESTORE));
  if (copied < done)
    HIP_TRY(hipMemcpyAsync(trace_out + 3 * copied, c->refine_trace + 3 * copied, (size_t)3 * (done - copied) * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  *n_done_out = done;
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// F_n, the entropy of q_n, the best column and the latent counts of the resident lpj rows and K^n (kernels_refine.hpp).
// Reads rows and states only: valid after a seed, an upload or a pass alike; nothing of the EM state changes.
extern "C" int evoamd_posterior_scores(evoamd_ctx *c, double *F_out, double *entropy_out, int32_t *best_out,
                                       int32_t *k_best_out, double *k_mean_out) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  const size_t N = (size_t)c->N;
  TRY(c->score_buf.ensure(c, 4 * N));  // F | entropy | k_mean | best, k_best (int32)
  double *dF = c->score_buf, *dE = dF + N, *dK = dF + 2 * N;
  int *dbest = (int *)(dF + 3 * N), *dkbest = dbest + N;
  {
    SpanGuard g(c, KID_MISC);
    posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(
        c->lpj, c->states, c->N, c->L, c->S, c->S_perm, c->HW, F_out ? dF : nullptr, entropy_out ? dE : nullptr,
        best_out ? dbest : nullptr, k_best_out ? dkbest : nullptr, k_mean_out ? dK : nullptr);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "posterior scores");
  }
  if (F_out) HIP_TRY(hipMemcpyAsync(F_out, dF, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (entropy_out) HIP_TRY(hipMemcpyAsync(entropy_out, dE, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (k_mean_out) HIP_TRY(hipMemcpyAsync(k_mean_out, dK, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (best_out) HIP_TRY(hipMemcpyAsync(best_out, dbest, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (k_best_out) HIP_TRY(hipMemcpyAsync(k_best_out, dkbest, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// the dictionary resized: K^n in a new latent numbering (kernels_remap.hpp has the law)
// ---------------------------------------------------------------------------------------
// Writes into context-owned scratch and remembers (N, S, H_new) with it; the resident K^n, the lpj rows and every flag
// stay as they are.  Every refusal comes before anything is launched or allocated.
extern "C" int evoamd_remap_latents(evoamd_ctx *c, const int32_t *index, int H_new, int32_t *n_replaced_out, int64_t *sum_out) {
  REQUIRE(c && c->configured, "evoamd_remap_latents: nothing is resident (configure and upload, initialise or seed K^n first)");
  REQUIRE_KN(c);
  REQUIRE(index, "evoamd_remap_latents: index is NULL");
  REQUIRE(H_new >= 1 && H_new <= DIG_MAX_H, "evoamd_remap_latents: H_new must be in [1, 16384] (the digests' latent indices)");
  const int H = c->H, S = c->S, bg = c->bg_unit ? 1 : 0;
  {
    std::vector<uint8_t> seen((size_t)H, 0);
    for (int h = 0; h < H_new; h++) {
      const int v = index[h];
      if (v == -1) continue;
      if (v < 0 || v >= H)
        return fail(EVOAMD_E_INVALID, "evoamd_remap_latents: index[%d] = %d is out of range (-1 or a source latent in [0, %d))", h, v, H);
      if (seen[v]) return fail(EVOAMD_E_INVALID, "evoamd_remap_latents: duplicate source latent %d (index[%d])", v, h);
      seen[v] = 1;
    }
  }
  if (bg) {
    if (index[H_new - 1] != H - 1)
      return fail(EVOAMD_E_INVALID, "evoamd_remap_latents: with the background unit the last index must be H - 1 = %d (it is %d)",
                  H - 1, index[H_new - 1]);
  }
  const i64 Hv2 = H_new - bg;
  if (Hv2 * (Hv2 + 1) / 2 < S)
    return fail(EVOAMD_E_INVALID,
                "evoamd_remap_latents: Hv' (Hv' + 1) / 2 = %lld fill candidates are fewer than S = %d states (Hv' = %lld): such "
                "shapes belong to init_states", (long long)(Hv2 * (Hv2 + 1) / 2), S, (long long)Hv2);
  const int HW = c->HW, HW2 = (H_new + 63) / 64;
  int W = REMAP_WAVES;
  while (W > 1 && remap_lds_words(W, S, HW, HW2) * sizeof(u64) > REMAP_LDS_BYTES) W >>= 1;
  if (remap_lds_words(W, S, HW, HW2) * sizeof(u64) > REMAP_LDS_BYTES)
    return fail(EVOAMD_E_INVALID,
                "evoamd_remap_latents: S = %d states of %d + %d words and their digests do not fit one wavefront's LDS slice "
                "(the cap at these H, H_new is S = %d)", S, HW, HW2, (int)((REMAP_LDS_BYTES / 8 - 32 * HW2) / (HW + HW2 + 1)));
  HIP_TRY(hipSetDevice(c->device));
  const size_t N = (size_t)c->N;
  made_remap(c, 0, 0, 0);  // whatever an earlier remap left is overwritten from here on
  TRY(c->remap_states.ensure(c, N * S * HW2));
  TRY(c->remap_dig.ensure(c, N * S));
  TRY(c->remap_i.ensure(c, (size_t)H_new + N));
  TRY(c->remap_sum.ensure(c, 1));
  HIP_TRY(hipMemcpyAsync(c->remap_i, index, (size_t)H_new * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->remap_sum, 0, sizeof(unsigned long long), c->stream));
  RemapArgs a;
  a.src = c->states;
  a.index = c->remap_i;
  a.dst = c->remap_states;
  a.dig = c->remap_dig;
  a.n_replaced = c->remap_i + H_new;
  a.sum = c->remap_sum;
  a.N = c->N;
  a.S = S;
  a.S_perm = c->S_perm;
  a.H = H;
  a.HW = HW;
  a.H2 = H_new;
  a.HW2 = HW2;
  a.Hv2 = (int)Hv2;
  a.bg = bg;
  {
    const unsigned grid = (unsigned)std::min<i64>(cdiv(c->N, W), (i64)c->n_cu * 16);
    SpanGuard g(c, KID_REMAP);
    remap_latents_kernel<<<grid, 64 * W, remap_lds_words(W, S, HW, HW2) * sizeof(u64), c->stream>>>(a);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "remap latents");
  }
  unsigned long long sum = 0;
  if (n_replaced_out) HIP_TRY(hipMemcpyAsync(n_replaced_out, a.n_replaced, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&sum, c->remap_sum, sizeof(sum), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (sum_out) *sum_out = (int64_t)sum;
  made_remap(c, c->N, S, H_new);
  return 0;
}

// After the caller has configured the context for H_new: the scratch becomes the resident K^n (a swap of the buffers), as
// if the caller had uploaded it; the scratch is released, so a second adopt without a new remap is refused.
extern "C" int evoamd_adopt_remapped_states(evoamd_ctx *c) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(c->remap_H > 0, "evoamd_adopt_remapped_states: no remapped states to adopt (evoamd_remap_latents first; an adopt uses them up)");
  if (c->N != c->remap_N || c->S != c->remap_S || c->H != c->remap_H)
    return fail(EVOAMD_E_INVALID,
                "evoamd_adopt_remapped_states: the context is configured for (N, S, H) = (%lld, %d, %d), the remapped states are "
                "(%lld, %d, %d)", (long long)c->N, c->S, c->H, (long long)c->remap_N, c->remap_S, c->remap_H);
  REQUIRE(c->dig && c->remap_states.size() >= c->states.size() && c->remap_dig.size() >= c->dig.size(),
          "evoamd_adopt_remapped_states: the scratch does not cover the geometry");
  HIP_TRY(hipSetDevice(c->device));
  TRY(sync_streams(c));  // a prefetched pass may still read the old buffers
  std::swap(c->states, c->remap_states);
  std::swap(c->dig, c->remap_dig);
  c->remap_states.reset();
  c->remap_dig.reset();
  made_remap(c, 0, 0, 0);
  on_kn_changed(c, KN_BY_CALLER);
  on_kn_complete(c);
  return 0;
}

// ---------------------------------------------------------------------------------------
// K^n resized: S changes, the best states stay, new slots are filled near the best (kernels_resize.hpp has the law)
// ---------------------------------------------------------------------------------------
// Writes into context-owned scratch and remembers (N, S_new, H) with it; the resident K^n, the lpj rows and every flag
// stay as they are.  Every refusal comes before anything is launched or allocated.
extern "C" int evoamd_resize_states(evoamd_ctx *c, int S_new, int32_t *src_slot_out) {
  REQUIRE(c && c->configured, "evoamd_resize_states: nothing is resident (configure and upload, initialise or seed K^n first)");
  REQUIRE_KN(c);
  REQUIRE(c->lpj_kn_gen == c->kn_gen,
          "evoamd_resize_states: the lpj rows are not those of the resident K^n (evoamd_lpj_resident or evoamd_upload_lpj first)");
  const int S = c->S, H = c->H, HW = c->HW, bg = c->bg_unit ? 1 : 0;
  REQUIRE(S_new >= 1, "evoamd_resize_states: S_new must be positive");
  REQUIRE(c->dig && H <= DIG_MAX_H, "evoamd_resize_states: H must be at most 16384 (the digests' latent indices)");
  if (S_new == S) return fail(EVOAMD_E_INVALID, "evoamd_resize_states: S_new = %d is the resident S: nothing to resize", S_new);
  if (S_new > RESIZE_MAX_S || S > RESIZE_MAX_S)
    return fail(EVOAMD_E_INVALID, "evoamd_resize_states: S = %d -> S_new = %d: at most %d states per datapoint are supported",
                S, S_new, RESIZE_MAX_S);
  const i64 Hv = H - bg;
  if (S_new > S && Hv * (Hv + 1) / 2 - 1 < S_new)
    return fail(EVOAMD_E_INVALID,
                "evoamd_resize_states: Hv (Hv + 1) / 2 - 1 = %lld neighbours of the best state are fewer than S_new = %d states "
                "(Hv = %lld)", (long long)(Hv * (Hv + 1) / 2 - 1), S_new, (long long)Hv);
  int W = RESIZE_WAVES;
  const size_t share = resize_lds_words(S, S_new, HW) * sizeof(u64);
  while (W > 1 && W * share > RESIZE_LDS_BYTES) W >>= 1;
  if (share > RESIZE_LDS_BYTES)
    return fail(EVOAMD_E_INVALID, "evoamd_resize_states: the keys of S = %d states, %d words of the best state and the list of "
                "S_new = %d slots (%zu bytes) do not fit one wavefront's share of LDS", S, HW, S_new, share);
  HIP_TRY(hipSetDevice(c->device));
  const size_t N = (size_t)c->N;
  FitList scratch;  // does it fit?  Decided before anything is released, allocated or launched.
  scratch.add(c->resize_states, N * S_new * HW);
  scratch.add(c->resize_dig, N * S_new);
  scratch.add(c->resize_src, N * S_new);
  size_t avail;
  TRY(scratch.measure(avail));
  if (scratch.grow > avail)
    return fail(EVOAMD_E_INVALID, "evoamd_resize_states: the resized K^n needs %zu bytes of device memory, %zu are free", scratch.grow,
                avail);
  made_resize(c, 0, 0, 0);  // whatever an earlier resize left is overwritten from here on
  TRY(scratch.ensure_all(c));
  ResizeArgs a;
  a.src = c->states;
  a.lpj = c->lpj;
  a.dst = c->resize_states;
  a.dig = c->resize_dig;
  a.src_slot = c->resize_src;
  a.err = c->err;
  a.N = c->N;
  a.S = S, a.S2 = S_new, a.S_perm = c->S_perm, a.L = c->L;
  a.H = H, a.HW = HW, a.Hv = (int)Hv, a.bg = bg;
  {
    const unsigned grid = (unsigned)std::min<i64>(cdiv(c->N, W), (i64)c->n_cu * 16);
    SpanGuard g(c, KID_RESIZE);
    resize_states_kernel<<<grid, 64 * W, W * share, c->stream>>>(a);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "resize states");
  }
  if (src_slot_out) HIP_TRY(hipMemcpyAsync(src_slot_out, a.src_slot, N * S_new * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  TRY(check_err(c));  // (waits for the stream)
  made_resize(c, c->N, S_new, H);
  return 0;
}

// After the caller has configured the context for (N, H, S_new): the scratch becomes the resident K^n (a swap of the
// buffers), as if the caller had uploaded it; the scratch is released, so a second adopt without a new resize is refused.
extern "C" int evoamd_adopt_resized_states(evoamd_ctx *c) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(c->resize_S > 0, "evoamd_adopt_resized_states: no resized states to adopt (evoamd_resize_states first; an adopt uses them up)");
  if (c->N != c->resize_N || c->S != c->resize_S || c->H != c->resize_H)
    return fail(EVOAMD_E_INVALID,
                "evoamd_adopt_resized_states: the context is configured for (N, S, H) = (%lld, %d, %d), the resized states are "
                "(%lld, %d, %d)", (long long)c->N, c->S, c->H, (long long)c->resize_N, c->resize_S, c->resize_H);
  REQUIRE(c->dig && c->resize_states.size() >= c->states.size() && c->resize_dig.size() >= c->dig.size(),
          "evoamd_adopt_resized_states: the scratch does not cover the geometry");
  HIP_TRY(hipSetDevice(c->device));
  TRY(sync_streams(c));  // a prefetched pass may still read the old buffers
  std::swap(c->states, c->resize_states);
  std::swap(c->dig, c->resize_dig);
  c->resize_states.reset();
  c->resize_dig.reset();
  c->resize_src.reset();
  made_resize(c, 0, 0, 0);
  on_kn_changed(c, KN_BY_CALLER);
  on_kn_complete(c);
  return 0;
}

// counts_out[h] = datapoints whose MAP state (first column of maximal lpj) has latent h on.  Reads rows and states only,
// like evoamd_posterior_scores.
extern "C" int evoamd_latent_map_counts(evoamd_ctx *c, int64_t *counts_out) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(counts_out, "counts_out is NULL");
  REQUIRE_KN(c);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)64 * c->HW;
  TRY(c->map_counts.ensure(c, n));
  HIP_TRY(hipMemsetAsync(c->map_counts, 0, n * sizeof(unsigned long long), c->stream));
  {
    SpanGuard g(c, KID_MISC);
    latent_map_count_kernel<<<cdiv(c->N, MAPCOUNT_WAVES), 64 * MAPCOUNT_WAVES, 0, c->stream>>>(
        c->lpj, c->states, c->N, c->L, c->S, c->S_perm, c->HW, c->map_counts);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "latent map counts");
  }
  HIP_TRY(hipMemcpyAsync(counts_out, c->map_counts, (size_t)c->H * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// statistics
// ---------------------------------------------------------------------------------------
extern "C" int64_t evoamd_acc_size(evoamd_ctx *c) { return (c && c->configured) ? c->acc_n : -1; }

static int row_lse(evoamd_ctx *c, const double *lpj, i64 N, int L, double *rowmax, double *rowsum, double *out_slot) {
  const unsigned nb = cdiv(N, 4);
  TRY(c->partial.ensure(c, (size_t)3 * nb));
  TRY(c->partial2.ensure(c, nb));
  if (lpj != c->lpj) on_lpj_overwritten(c);  // the partial buffer now belongs to another matrix
  SpanGuard g(c, KID_ROW_LSE);
  row_lse_kernel<<<nb, 256, 0, c->stream>>>(lpj, N, L, rowmax, rowsum, c->partial);
  reduce_partials_kernel<<<1, 256, 0, c->stream>>>(c->partial, nb, out_slot, 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int compute_reconstruction(evoamd_ctx *c);

// the forked statistics contraction must have finished before anything reads its part of acc
static int join_fork(evoamd_ctx *c) {
  if (c->gemm_forked) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->gemm_forked = false;
  }
  if (c->ar_gemm_pending) {  // second piece of the split all-reduce (stats_compute sent the rest before the inverses)
    c->ar_gemm_pending = false;
    const AccLayout a = acc_layout(c);
    SpanGuard g(c, KID_ALLREDUCE);
    RCCL_TRY(g_rccl.AllReduce(c->acc + a.sWp, c->acc + a.sWp, (size_t)(a.y2 - a.sWp), /*ncclDouble*/ 8, /*ncclSum*/ 0,
                              c->comm, c->stream));
  }
  return 0;
}

static TailArgs make_tail_args(evoamd_ctx *c, const AccLayout &a, i64 N, bool census, int skipped) {
  TailArgs ta = {};
  ta.tail = c->acc + a.tail;
  ta.N = (double)N;
  ta.dpar = c->dpar;
  ta.flags = c->flags;
  ta.nflags3 = 3 * N;
  ta.nper = N;
  ta.err = c->err;
  ta.list_n = c->model == EVOAMD_MODEL_SSSC ? (census ? c->clist_n : c->list_n) : nullptr;
  ta.nshards = LIST_SHARDS;
  ta.skipped_mask = skipped;
  ta.census = c->census;
  ta.census_lists = census ? 1 : 0;
  ta.fly_n = (census && c->model == EVOAMD_MODEL_SSSC) ? c->list_n : nullptr;
  ta.fly_skip = c->pending_skip;
  return ta;
}

// flops of the K = N contraction of the statistics pass: [Y | Es | Ez]^T Ez (ES3C), Es^T Y (EBSC)
static double contraction_flops(const evoamd_ctx *c) {
  return c->model == EVOAMD_MODEL_SSSC ? 2.0 * (double)c->N * (c->D + 2.0 * c->H) * c->H : 2.0 * (double)c->N * c->D * c->H;
}

// What a statistics pass decides before it enqueues anything (stats_plan); the stages only read it.
struct StatsPlan {
  AccLayout a;
  i64 N;
  int H, D;
  bool masked;              // incomplete data
  LevelHints lv;            // how much is known about the final K^n (resident states and accepted candidates)
  bool gemm_timed;          // a class on the main stream is being timed: no second stream
  double gemm_flops;
  bool pays;       // the contraction is worth a second stream (agreed over the ranks)
  bool early;      // its stream branches off behind the last writer of the rows, not behind the finish kernel
  bool fork_gemm;  // the contraction is still running when stats_compute returns; the caller joins
  i64 rpb;         // datapoints per column-sum partial
  int nblk;        // number of those
  int nchunks;     // blocks of datapoints, each followed by its part of the contraction
  i64 rows_per_chunk;
  bool second_stream;
  int gemm_spare;  // workgroups per XCD the forked contraction leaves to the Theta chain where "sk_spare" is automatic
  int waves;       // waves per workgroup of the ES3C wave-per-datapoint kernel
  bool census;     // ES3C: the levels read the census lists
  bool bsc_wave;   // EBSC: the wave-per-datapoint kernel (else the round-1 kernel + column-sum pass)
  bool kappa;      // ES3C: the kappa route -- the main kernel reads the lpj pass's kappa records instead of B rows and tables
};

// One block of datapoints: rows [n0, n0 + nc) = column-sum partials [blk0, blk0 + nblk_c)
struct StatsBlock {
  int ci;
  i64 n0, nc;
  int blk0, nblk_c;
};

// What a later stage of the pass learns from an earlier one.
struct StatsFlow {
  bool early_recorded = false;  // the contraction's branch point has been recorded (rows_written)
  bool tail_done = false;       // the accumulator tail rode in the finish launch
  bool served3 = false;  // the wavefront level ran on list 3 although the census did not ask for it (exact-mode hand-over)
  int skipped = 0;       // levels not launched: their input lists must be found empty
  int bsc_grid = 0;      // grid of the EBSC wave kernel = number of its sigma partials
  PairBins bsc_pb = {};  // EBSC: the bins its wave kernel appended to
  PairBins pb = {};      // ES3C: the bins of this pass (re-cut for the flat kernel)
};

// ES3C: argument block shared by the scatter kernels, the levels K^n needs and the on-the-fly lists
struct Es3cPass {
  double *Es, *Ez, *Ed;  // columns of [Y | Es | Ez | Ed] (ES3C)
  SsscArgs sa = {};
  bool need[3] = {true, true, true};
  Es3cLists ls = {};  // (census mode means one block, so the census lists are read with the pass's capacity too)
};

// ES3C on complete data, one block: its rows of the argument block, its share of the counts, the form of its main kernel
struct Es3cBlock {
  SsscArgs sc;
  i64 total;
  LevelHints lv;  // the pass's, scaled to the block's share of the datapoints
  int flatG = 0;  // census mode, thread-per-state form of the main kernel: G datapoints per 1024-thread workgroup and round
  size_t flat_lds = 0;
  bool few4;  // few states above four latents: no quad launch for them, the wavefront kernel behind the main kernel adds them
};

// Pair bins (asked once per pass and model): they pay when the fixed cost of the reduce pass (zero + store nb x PB_NSH
// tiles, ~20 us) is less than the global atomics they absorb -- from ~256k resident states on (N = 12.5k x S = 200:
// statistics pass 0.63 -> 0.40 ms).  ES3C needs complete data as well, EBSC its wave kernel.
// Not a member of StatsPlan: ensure_bins_capacity, in the preamble of the pass, may re-cut or drop c->pbins.
static bool stats_bins_pay(const evoamd_ctx *c) {
  return c->pbins.ent && (c->pair_bins == 2 || (c->pair_bins == 1 && c->N * (i64)c->S >= (i64)c->bins_min * 1024));
}

// resident workgroups per CU of a wave-per-datapoint statistics kernel: what its LDS leaves, the CU's waves, 1 .. 8
static int stats_per_cu(size_t lds_per_wg, int wave_lim) {
  int per_cu = (int)((160 * 1024) / lds_per_wg);
  if (per_cu > wave_lim) per_cu = wave_lim;
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  return per_cu;
}

// every kernel that writes the E_q rows of the (only) block has been enqueued: the contraction's stream branches off here
static int rows_written(evoamd_ctx *c, const StatsPlan &p, StatsFlow &fl) {
  if (p.second_stream && p.nchunks == 1 && p.early && !p.masked) {
    HIP_TRY(hipEventRecord(c->ev_chunk[0], c->stream));
    fl.early_recorded = true;
  }
  return 0;
}

// incomplete data: y_hat = E W^T under the Theta of this E-step, and y_reconstructed from it -- the rows the Wp
// contraction reads.  `asked_msg`: ES3C requires rec_in_stats, and says so between the two launches.
static int reconstruct_rows(evoamd_ctx *c, const char *asked_msg = nullptr) {
  TRY(compute_reconstruction(c));
  if (asked_msg) REQUIRE(c->rec_in_stats, asked_msg);
  select_rec_kernel<<<cdiv(c->N, 4), 256, 0, c->stream>>>(c->Y, c->ldY, c->mask_x, c->mask_infr, c->yhat, c->N, c->D, c->Yrec,
                                                          c->model == EVOAMD_MODEL_BSC);
  HIP_TRY(hipGetLastError());
  made_yrec_from_pass(c, /*in_stats=*/true);
  return 0;
}

// Fills the plan from the context as it is at entry.  Enqueues nothing; with a communicator it may talk to the other
// ranks once per geometry (pays_agreed), at the same point on every rank.
static int stats_plan(evoamd_ctx *c, bool fork_gemm, StatsPlan &p) {
  p = StatsPlan{};
  p.a = acc_layout(c);
  p.N = c->N;
  p.H = c->H;
  p.D = c->D;
  p.masked = c->mask_infr != nullptr;
  p.lv.known_tag = c->cand_from_device ? 1 : 2;
  p.lv.one_bit = c->cand_from_device;
  // (the contraction's own class alone does not count: its span is recorded on the stream the product runs on, so it
  // can be timed forked, as the timed loop runs it -- bench.py's `mfma` block)
  p.gemm_timed = c->timing && (c->timing_mask & ((1u << KID_MSTEP) | (1u << KID_MISC) |
                                                 (1u << KID_STATS) | (1u << KID_STATS_OVF)));
  // the K = N contraction is worth a second stream when it is big (measured, tools/ab.sh, MI355X: ES3C H = 512 gains;
  // ES3C H = 128 and the EBSC shapes at N <= 50k lose ~1 %: the fork / join events cost ~10 us)
  const double gemm_flops = p.gemm_flops = contraction_flops(c);
  // (EBSC: from ~5e10 flops on and without a communicator -- c5 on one GPU 6.47 -> 6.24 ms per iteration with eight
  // slots per XCD left to its 32 block steps of 256 workgroups; its accumulator is all-reduced in one piece)
  bool pays = (c->model == EVOAMD_MODEL_SSSC && gemm_flops >= 8e9) || (c->model == EVOAMD_MODEL_BSC && !c->comm && gemm_flops >= 5e10);
  // branching off early (option "early_fork") makes the fork pay for small ES3C products too: the product then runs
  // beside the pair-bin reduce, the finish kernel and the register-resident inverse instead of in front of them
  const bool early = p.early = c->early_fork == 1 || (c->early_fork < 0 && gemm_flops < 2e10);
  if (c->model == EVOAMD_MODEL_SSSC && !c->comm && early && gemm_flops >= 5e8 && !c->mask_infr) pays = true;
  // EBSC the same (c3: the 48 us product beside the reduce, the finish kernel and the 9-launch elimination chain) where
  // the wave-per-datapoint statistics kernel runs (the branch point sits behind it)
  if (c->model == EVOAMD_MODEL_BSC && !c->comm && early && gemm_flops >= 5e8 && !c->mask_infr && c->bsc_wave_opt &&
      dig_for(c, c->states) && cdiv(c->S, 64) <= 4 && (size_t)5 * c->H * sizeof(double) <= 150 * 1024 && !c->f32)
    pays = true;
  if (c->comm && c->model == EVOAMD_MODEL_SSSC) {
    // np.array_split shards differ by one row, so a shard size next to the threshold would make some ranks
    // issue three all-reduces and others one: agree once per geometry (max over ranks), same call on every rank
    if (c->pays_agreed < 0) {
      double v = pays ? 1.0 : 0.0;
      TRY(evoamd_comm_allreduce_host(c, &v, 1, 1));
      c->pays_agreed = v > 0.0 ? 1 : 0;
    }
    pays = c->pays_agreed == 1;
  }
  p.pays = pays;
  // fork_gemm: the contraction is still running when this function returns (beside the H x H inverses); the caller
  // joins.  With a communicator only ES3C does that (its accumulator is all-reduced in pieces).
  p.fork_gemm = fork_gemm && (c->overlap_gemm == 2 || (c->overlap_gemm == 1 && pays)) &&
                (!c->comm || c->model == EVOAMD_MODEL_SSSC) && !p.gemm_timed && !c->mask_infr;
  // column-sum partials: at most ~128 of them (the finish kernels add them serially per column); a multiple of
  // four rows so that a block boundary is a workgroup boundary of the EBSC kernel (four datapoints each)
  p.rpb = ((std::max<i64>(256, cdiv(p.N, 128)) + 3) / 4) * 4;
  p.nblk = (int)cdiv(p.N, p.rpb);
  // Blocks of datapoints: the scatter kernels of block i + 1 (bound by the f64 atomic rate, executed at the memory
  // side) run beside the MFMA contraction of block i on the second stream.  Same kernels, same sums; the
  // contraction accumulates with its atomic epilogue.  Not while the classes involved are being timed one by one.
  int nchunks = 1;
  if (!p.masked && !p.gemm_timed && c->overlap_gemm != 0 && c->stats_chunks > 1 && (gemm_flops >= 8e9 || c->overlap_gemm == 2))
    nchunks = std::min<int>(c->stats_chunks, p.nblk);
  // census lists need the 4-wave statistics kernel (rows of four datapoints + column sums in LDS: 11 H doubles); larger
  // H -- or a waves-per-workgroup measurement option -- takes the round-2 level chains, decided BEFORE any level runs
  // (8 / 16 waves per workgroup were measured: c4 8 waves -4 %, 16 waves 2x slower; c2 16 waves 112 vs 74 us)
  p.waves = (c->stats_waves == 4 || c->stats_waves == 8 || c->stats_waves == 16)
                ? c->stats_waves  // measurement option
                : ((size_t)(4 * 2 + 3) * p.H * sizeof(double) <= 150 * 1024 ? 4 : 1);
  p.census = census_mode(c) && !p.masked && p.waves == 4;
  if (p.census) nchunks = 1;  // the census lists cover the whole shard
  // kappa route (option "stats_kappa"): census lists + the four-wave kernel with staging on (not a measurement form of
  // it), and records written under this gen for this K^n (or carried into it by the selection)
  p.kappa = p.census && kappa_shape_ok(c) && c->kap_gen == c->gen && !c->stats_flat && c->stats_stage != 0 &&
            (c->stats_waves == 0 || c->stats_waves == 4);
  p.rows_per_chunk = (i64)cdiv(p.nblk, nchunks) * p.rpb;
  p.nchunks = nchunks = (int)cdiv(p.N, p.rows_per_chunk);
  p.second_stream = p.fork_gemm || nchunks > 1;
  // Forked beside the elimination chain: a resident-sized grid holds every workgroup slot until it has drained, and the
  // grouped split-K drains all at once -- the chain (H / 32 block steps of 128 workgroups each) then runs entirely BEHIND
  // the product (0.25 ms at the north-star shape).  Four slots per XCD left free (34 tiles x 14 chunks = 476 workgroups
  // instead of 510) cost the product 6 % and let the chain finish well inside it.  Measured (interleaved A/B, ms per
  // iteration): c4 3.90 -> 3.82, N / 2 2.31 -> 2.16 (8 slots: 2.22), N / 4 1.54 -> 1.45 with 4 and 1.41 with 8, N / 8
  // 1.14 -> 1.09 with 4 and 1.065 with 8 (12 / 16: the same): 4 where the product is long against the chain, else 8.
  {
    const double chain_us = c->H >= 256 ? 15.0 * cdiv(c->H, 32) : 8.5 * cdiv(c->H, 16);
    p.gemm_spare = !(p.fork_gemm && nchunks == 1) ? 0 : ((gemm_flops / 65e6 >= 3.0 * chain_us && c->H <= 512) ? 4 : 8);
  }
  // EBSC: wave-per-datapoint kernel with prefetch, pair bins and in-kernel column sums where it applies (digests, S <= 256,
  // one block); else the round-1 kernel + column-sum pass
  const int SRb = (int)cdiv(c->S, 64);
  p.bsc_wave = c->model == EVOAMD_MODEL_BSC && c->bsc_wave_opt && dig_for(c, c->states) &&
               (SRb == 1 || SRb == 2 || SRb == 4 || SRb == 3) && nchunks == 1 && (size_t)5 * p.H * sizeof(double) <= 150 * 1024;
  return 0;
}

// ---- EBSC producer of the (only) block: the wave-per-datapoint kernel and the reduce of its pair bins
static int stats_bsc_wave(evoamd_ctx *c, const StatsPlan &p, const StatsBlock &blk, StatsFlow &fl) {
  const AccLayout &a = p.a;
  const i64 nc = blk.nc;
  const int H = p.H;
  const u64 *bdig = dig_for(c, c->states);
  const int SRb = (int)cdiv(c->S, 64);
  SpanGuard g(c, KID_STATS);
  const size_t ldsb = (size_t)5 * H * sizeof(double);
  const int per_cu = stats_per_cu(ldsb + 2048, 8);  // (four waves per workgroup)
  PairBins &bsc_pb = fl.bsc_pb;
  bsc_pb = PairBins{};
  if (stats_bins_pay(c)) bsc_pb = c->pbins;
  int sgrid = (int)std::min<i64>(cdiv(nc, 4), (i64)c->n_cu * per_cu * 2);
  if (sgrid > 2048) sgrid = 2048;  // the size of the sigma partials
  if (bsc_pb.ent && sgrid > bsc_pb.nwg) sgrid = bsc_pb.nwg;  // one private region per producer workgroup and bin
  PB_GRID_CHECK(bsc_pb, sgrid);
  if (bsc_pb.ent) on_bins_append(c);
  fl.bsc_grid = sgrid;
  void *EsP = c->f32 ? (void *)c->Esf : (void *)c->Es;
  double *csb = c->acc_base + 4;
#define BSC_WAVE(SR)                                                                                                      \
  bsc_stats_wave_kernel<SR><<<sgrid, 256, ldsb, c->stream>>>(c->states, c->lpj, c->rowmax, c->rowsum, c->yy, nc, c->S,     \
                                                            c->S_perm, H, c->HW, c->dpar, EsP, c->acc + a.Wq, c->partial2, \
                                                            bdig, c->f32 ? 1 : 0, bsc_pb, csb)
  if (SRb == 1) BSC_WAVE(1);
  else if (SRb == 2) BSC_WAVE(2);
  else BSC_WAVE(4);
#undef BSC_WAVE
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "bsc stats (wave)");
  TRY(rows_written(c, p, fl));  // the E_q[s] rows are written: the product may start
  if (bsc_pb.ent) {
    pair_bins_reduce_kernel<3><<<bsc_pb.nb * bsc_pb.nsh, PB_RTHREADS, (size_t)3 * 2 * bsc_pb.rf * H * sizeof(double), c->stream>>>(
        bsc_pb, H, 0);
    HIP_TRY(hipGetLastError());
    made_bins_clean(c);
  }
  return 0;
}

// ---- EBSC producers of one block: the round-1 kernel + column-sum pass
static int stats_bsc_classic(evoamd_ctx *c, const StatsPlan &p, const StatsBlock &blk) {
  const AccLayout &a = p.a;
  const i64 n0 = blk.n0, nc = blk.nc;
  const int H = p.H;
  {
    SpanGuard g(c, KID_STATS);
    with_hw(c->HW, [&](auto hw) {
      bsc_stats_kernel<decltype(hw)::value><<<cdiv(nc, 4), 256, (size_t)4 * H * sizeof(double), c->stream>>>(
          c->states + (size_t)n0 * c->S * c->HW, c->lpj + (size_t)n0 * c->L, c->rowmax + n0, c->rowsum + n0, c->yy + n0, nc,
          c->S, c->S_perm, H, c->HW, c->dpar,
          c->f32 ? (void *)(c->Esf + (size_t)n0 * H) : (void *)(c->Es + (size_t)n0 * H), c->acc + a.Wq, c->partial2 + n0 / 4,
          dig_for(c, c->states) ? dig_for(c, c->states) + (size_t)n0 * c->S : nullptr, c->f32 ? 1 : 0);
    });
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "bsc stats");
  }
  {
    SpanGuard g(c, KID_MISC);
    if (c->f32)
      colsum_partial_f32_kernel<<<dim3(cdiv(H, 64), blk.nblk_c), 256, 0, c->stream>>>(c->Esf + (size_t)n0 * H, H, nc, H, p.rpb,
                                                                                      c->colpart + (size_t)blk.blk0 * H);
    else
      colsum_partial_kernel<<<dim3(cdiv(H, 64), blk.nblk_c), 256, 0, c->stream>>>(c->Es + (size_t)n0 * H, H, nc, H, p.rpb,
                                                                                  c->colpart + (size_t)blk.blk0 * H);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// ---- EBSC producers of one block, then (incomplete data) the rows the Wp contraction reads instead of Y
static int stats_bsc_block(evoamd_ctx *c, const StatsPlan &p, const StatsBlock &blk, StatsFlow &fl, const double *&Ywp, int &ldwp) {
  TRY(p.bsc_wave ? stats_bsc_wave(c, p, blk, fl) : stats_bsc_classic(c, p, blk));
  if (p.masked) {  // incomplete data: the Wp contraction reads y_reconstructed (bsc.py:184-189,211); one block only
    if (c->rec_in_stats) {
      TRY(reconstruct_rows(c));  // y_hat = Es W^T under the Theta of this E-step (_models.py:193-194)
    }
    REQUIRE(c->yrec_valid, "incomplete data: the M-step needs y_reconstructed (bsc.py:186); reconstruct or upload it");
    Ywp = c->Yrec;
    ldwp = p.D;
  }
  return 0;
}

// ---- ES3C on incomplete data (sssc.py:276: W[this_x_infr, :]): the state terms belong to the datapoint, so every
// state goes through the wavefront kernel, which forms W_obs^T W_obs itself and ADDS its moments to the rows (they
// start from zero here)
static int stats_sssc_masked_block(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep) {
  const i64 N = p.N;
  const int H = p.H;
  const i64 total = N * (i64)c->S;
  HIP_TRY(hipMemset2DAsync(ep.Es, (size_t)c->ldY * sizeof(double), 0, (size_t)3 * H * sizeof(double), (size_t)N, c->stream));
  {
    SpanGuard g(c, KID_STATS);
    sssc_big_kernel<1><<<(int)std::min<i64>(total, 65536), 64, big_lds(8), c->stream>>>(ep.sa, ep.ls.none_in, ep.ls.o3, 8);
    sssc_big_kernel<1><<<1024, 64, big_lds(SSSC_KCAP), c->stream>>>(ep.sa, ep.ls.i3, ep.ls.none_out, SSSC_KCAP);
    HIP_TRY(hipGetLastError());
  }
  SpanGuard g(c, KID_MISC);
  colsum_partial_kernel<<<dim3(cdiv(3 * H, 64), p.nblk), 256, 0, c->stream>>>(ep.Es, c->ldY, N, 3 * H, p.rpb, c->colpart);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ES3C on complete data: this block's rows of the argument block, its level hints and the form of its main kernel
static Es3cBlock sssc_block_setup(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const StatsBlock &blk) {
  const SsscArgs &sa = ep.sa;
  const i64 n0 = blk.n0;
  const int H = p.H, D = p.D;
  Es3cBlock eb = {};
  SsscArgs &sc = eb.sc;
  sc = sa;  // this block's rows
  sc.states = sa.states + (size_t)n0 * c->S * c->HW;
  if (sa.dig) sc.dig = sa.dig + (size_t)n0 * c->S;
  sc.Bm = sa.Bm + (size_t)n0 * H;
  sc.yy = sa.yy + n0;
  sc.lpj_in = sa.lpj_in + (size_t)n0 * sa.ldo;
  sc.rowmax = sa.rowmax + n0;
  sc.rowsum = sa.rowsum + n0;
  sc.Es = sa.Es + (size_t)n0 * sa.ldE;
  sc.Ez = sa.Ez + (size_t)n0 * sa.ldE;
  sc.Ed = sa.Ed + (size_t)n0 * sa.ldE;
  sc.N = blk.nc;
  eb.total = blk.nc * (i64)c->S;
  eb.lv = p.lv;
  eb.lv.scale = (double)blk.nc / (double)p.N;
  if (p.census && c->stats_flat && c->S <= FLAT_T && (H % 2) == 0 && (D % 2) == 0 && sc.Ez == sc.Es + H && c->stats_waves == 0) {
    int flatG = FLAT_T / c->S;
    const int gmax = (int)(((size_t)140 * 1024 / sizeof(double) - (size_t)7 * H) / ((size_t)4 * H + 4));
    if (flatG > gmax) flatG = gmax;
    if (flatG > 4 * FLAT_T / H) flatG = 4 * FLAT_T / H;  // the round's B rows: at most two 16-byte pieces per thread
    if (flatG >= 1) eb.flat_lds = ((size_t)H * (4 * flatG + 7) + 4 * flatG) * sizeof(double);
    eb.flatG = flatG;
  }
  eb.few4 = p.census && eb.flatG < 1 && few_above4(c, eb.lv);
  return eb;
}

// ---- census mode, the quad levels FIRST: records of the listed states (read back by the wave-per-datapoint kernel), their
// diagonal second moments into the column-sum slices, their pairs into the bins (regions shared by workgroup index)
static int stats_sssc_census_quads(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const Es3cBlock &eb, StatsFlow &fl) {
  const bool *need = ep.need;
  const PairBins &pb = fl.pb;
  TRY(ensure_census(c));
  if (need[0] || need[1]) {
    SpanGuard g(c, KID_STATS_OVF);
    const unsigned gcap = pb.ent ? (unsigned)std::min(2048, pb.nwg) : 2048u;
    const size_t dl = (size_t)p.H * sizeof(double);
    // (the bins' region counters are zero here: pair_bins_reduce_kernel clears what it reads)
    if (need[0]) {
      SpanGuard gl(c, KID_STATS_K34);
      const unsigned qg = quad_grid(c, eb.lv, 0, eb.total, gcap);
      PB_GRID_CHECK(pb, qg);
      sssc_quad_kernel<1, 1, 2><<<qg, 256, dl, c->stream>>>(eb.sc, ep.ls.cA, ep.ls.none_out, ep.ls.o3, pb, c->ovf_rec);
    }
    if (need[1] && !eb.few4) {
      SpanGuard gl(c, KID_STATS_K58);
      const unsigned qg = quad_grid(c, eb.lv, 1, eb.total, gcap);
      PB_GRID_CHECK(pb, qg);
      sssc_quad_kernel<2, 1, 2><<<qg, 256, dl, c->stream>>>(eb.sc, ep.ls.cB, ep.ls.none_out, ep.ls.o3, pb, c->ovf_rec);
    }
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sssc stats quad levels");
  }
  return 0;
}

// ---- the main kernel of an ES3C block on complete data: thread-per-state (flat) or wave-per-datapoint
static int stats_sssc_main(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const Es3cBlock &eb, const StatsBlock &blk,
                           StatsFlow &fl) {
  const PairBins &pb = fl.pb;
  const SsscArgs &sc = eb.sc;
  const ListOut &o1 = ep.ls.o1;
  const i64 nc = blk.nc;
  const int H = p.H;
  const bool census = p.census;
  if (eb.flatG >= 1) {
    SpanGuard g(c, KID_STATS);
    int fgrid = (int)std::min<i64>(cdiv(nc, eb.flatG), (i64)c->n_cu);
    if (pb.ent && fgrid > pb.nwg) fgrid = pb.nwg;
    PB_GRID_CHECK(pb, fgrid);
    sssc_stats_flat_kernel<<<fgrid, FLAT_T, eb.flat_lds, c->stream>>>(sc, pb, c->ovf_rec, eb.flatG);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sssc stats main (flat)");
    return 0;
  }
  // one wave per datapoint, persistent workgroups: W x 2 H doubles of rows + 3 H of column accumulators in LDS
  const int Wv = p.waves;
  size_t lds = (size_t)(Wv * 2 + 3) * H * sizeof(double);
  const size_t lds_static = 1024 + (size_t)Wv * 512 + 128;  // the kernel's bin counters and overflow buffers
  REQUIRE(lds <= 150 * 1024, "ES3C statistics: H too large for the LDS rows (H <= 3800)");
  // B row of each wave's datapoint + the singleton table in LDS too when that still leaves two workgroups per CU
  const size_t lds_staged = lds + (size_t)(Wv + 4) * H * sizeof(double);
  const int stage = (H % 2) == 0 && 2 * (lds_staged + lds_static) <= 160 * 1024 && c->stats_stage != 0;
  if (stage) lds = lds_staged;
  const int per_cu = stats_per_cu(lds + lds_static, 32 / Wv);  // 32 waves per CU
  SpanGuard g(c, KID_STATS);
  if (p.kappa) {
    // kappa route: rows + four accumulator columns, no B rows and no tables in LDS
    SpanGuard gk(c, KID_STATS_KAPPA);
    const size_t ldk = (size_t)(4 * 2 + 4) * H * sizeof(double);
    const int per_cu_k = stats_per_cu(ldk + lds_static, 32 / 4);
    int kgrid = (int)std::min<i64>(cdiv(nc, 4), (i64)c->n_cu * per_cu_k * 4);
    if (pb.ent && kgrid > pb.nwg) kgrid = pb.nwg;
    PB_GRID_CHECK(pb, kgrid);
    sssc_stats_wave_kernel<1, 4, true, true><<<kgrid, 256, ldk, c->stream>>>(sc, o1, pb, 1, c->ovf_rec, eb.few4 ? 4 : 8);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sssc stats main (kappa)");
    return 0;
  }
  // a wave per datapoint while that is at most a few rounds of resident workgroups (a second datapoint per wave
  // doubles the kernel's critical path at small N), a persistent grid-stride loop beyond
  int sgrid = (int)std::min<i64>(cdiv(nc, Wv), (i64)c->n_cu * per_cu * 4);
  if (pb.ent && sgrid > pb.nwg) sgrid = pb.nwg;  // one private region per producer workgroup and bin
  PB_GRID_CHECK(pb, sgrid);
  auto wave4 = [&](auto hw) {
    constexpr int HWT = decltype(hw)::value;
    if (census)
      sssc_stats_wave_kernel<HWT, 4, true><<<sgrid, 256, lds, c->stream>>>(sc, o1, pb, stage, c->ovf_rec, eb.few4 ? 4 : 8);
    else
      sssc_stats_wave_kernel<HWT, 4><<<sgrid, 256, lds, c->stream>>>(sc, o1, pb, stage);
  };
  REQUIRE(!census || Wv == 4, "census lists need the 4-wave statistics kernel (option stats_waves)");
  if (Wv == 1) {
    sssc_stats_wave_kernel<0, 1><<<sgrid, 64, lds, c->stream>>>(sc, o1, pb, stage);
  } else if (Wv == 8) {
    sssc_stats_wave_kernel<0, 8><<<sgrid, 512, lds, c->stream>>>(sc, o1, pb, stage);
  } else if (Wv == 16) {
    sssc_stats_wave_kernel<0, 16><<<sgrid, 1024, lds, c->stream>>>(sc, o1, pb, stage);
  } else if (!stage || !sc.dig) {
    wave4(std::integral_constant<int, 0>{});
  } else {
    with_hw(c->HW, wave4);  // digests + staging: the instantiations that prefetch the next datapoint
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "sssc stats main");
  return 0;
}

// ---- the levels behind the main kernel, census form: resident states above eight latents + what the quads passed on
// (atomics)
static int stats_sssc_census_levels(evoamd_ctx *c, const Es3cPass &ep, const Es3cBlock &eb) {
  const bool *need = ep.need;
  if (need[0] || need[1] || need[2]) {
    SpanGuard g(c, KID_STATS_OVF);
    SpanGuard gl(c, KID_STATS_K9P);
    const int served = census_wavefront_levels<1, 2>(c, eb.sc, ep.ls, need, eb.few4, eb.lv, eb.total);
    on_levels_skipped(c, /*census_route=*/true, 0, served, true);  // (as in launch_sssc_lpj: nobody serves the on-the-fly list 2)
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sssc stats wavefront level (census)");
  }
  return 0;
}

// ---- the levels behind the main kernel, chains form: list 1 -> K = 4 -> list 2 -> K = 8 / wavefront -> list 3 -> wavefront
static int stats_sssc_chain_levels(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const Es3cBlock &eb, StatsFlow &fl) {
  const bool *need = ep.need;
  const PairBins &pb = fl.pb;
  const SsscArgs &sc = eb.sc;
  const i64 total = eb.total;
  const LevelHints &lv = eb.lv;
  if (need[0] || need[1] || need[2]) {
    SpanGuard g(c, KID_STATS_OVF);
    const size_t cs_lds = sc.cs ? (size_t)3 * p.H * sizeof(double) : 0;  // in-kernel column sums (LDS)
    bool merged23 = false;
    if (need[0]) {
      const unsigned g4 = pb_clamp(pb, level_grid(c, lv, 0, total, 1024, 256));
      PB_GRID_CHECK(pb, g4);
      sssc_small_kernel<4, 1, 2, 256><<<g4, 256, cs_lds, c->stream>>>(sc, ep.ls.i1, ep.ls.o2, pb, ep.ls.o3);
    }
    // (statistics mode of the K = 8 register kernel: 256 registers + 736 bytes of scratch per lane, one wave per
    // SIMD -- measured slower than the wavefront kernel at every size seen: 187 vs ~110 us at 5k states, 0.32
    // vs 0.25 ms for the pass's levels at the north-star shape; only when forced by option "sssc_k8" = 1)
    if (c->k8_mode == 1) {
      if (need[1]) {
        const unsigned g8 = pb_clamp(pb, level_grid(c, lv, 1, total, 256, 256));
        PB_GRID_CHECK(pb, g8);
        sssc_small_kernel<8, 1, 2, 256><<<g8, 256, cs_lds, c->stream>>>(sc, ep.ls.i2, ep.ls.o3, pb, ep.ls.o3);
      }
    } else if (need[1] && few_dense_states(c, lv)) {
      sssc_big_kernel<1><<<level_grid(c, lv, 1, total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
          sc, ep.ls.i2, ep.ls.none_out, SSSC_KCAP, ep.ls.i3);  // one launch for both wavefront levels (see lpj_sssc_round2_levels)
      fl.served3 = true;
      merged23 = true;
    } else if (need[1]) {
      sssc_big_kernel<1><<<level_grid(c, lv, 1, total * 256, 4096, 1), 64, big_lds(8), c->stream>>>(sc, ep.ls.i2, ep.ls.o3, 8);
    }
    if ((need[2] || c->sing_screen) && !merged23) {
      sssc_big_kernel<1><<<level_grid(c, lv, 2, total * 256, 1024, 1), 64, big_lds(SSSC_KCAP), c->stream>>>(
          sc, ep.ls.i3, ep.ls.none_out, SSSC_KCAP);
      fl.served3 = true;
    }
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sssc stats overflow levels");
  }
  return 0;
}

// ---- ES3C on complete data, one block: census quad levels, main kernel, the levels behind it, pair-bin reduce
static int stats_sssc_block(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const StatsBlock &blk, StatsFlow &fl,
                            bool debug_fail) {
  PairBins &pb = fl.pb;
  const Es3cBlock eb = sssc_block_setup(c, p, ep, blk);
  if (pb.ent) on_bins_append(c);  // this block's producers append; until its reduce (which zeroes the counters)
  if (blk.ci > 0) {  // the previous block's overflow census joins the running sum; fresh lists for this block
    census_lists_kernel<<<1, 256, 0, c->stream>>>(c->list_n, LIST_SHARDS, skip_mask(ep.need), c->err, c->census);
    HIP_TRY(hipGetLastError());
  }
  if (eb.flatG >= 1 && pb.ent) {
    // one resident workgroup per CU produces: the bins' entry space re-cut into n_cu regions per bin
    const i64 per_bin = (i64)pb.nwg * pb.cap;
    pb.nwg = std::min(pb.nwg, c->n_cu);
    pb.cap = (int)std::min<i64>(per_bin / pb.nwg, 1 << 30);
  }
  if (p.census) TRY(stats_sssc_census_quads(c, p, ep, eb, fl));
  TRY(stats_sssc_main(c, p, ep, eb, blk, fl));
  if (debug_fail)  // test hook: a pass that returns between its producers and the pair-bin reduce
    return fail(EVOAMD_E_INVALID, "debug_fail_stats: statistics pass stopped after its main kernel");
  TRY(p.census ? stats_sssc_census_levels(c, ep, eb) : stats_sssc_chain_levels(c, p, ep, eb, fl));
  TRY(rows_written(c, p, fl));
  if (pb.ent) {  // the entries of the main kernel and of the register-kernel levels: one tile pass per block
    SpanGuard g(c, KID_STATS);
    if (pb.planes == 4)
      pair_bins_reduce_kernel<4><<<pb.nb * pb.nsh, PB_RTHREADS, (size_t)4 * 2 * pb.rf * p.H * sizeof(double), c->stream>>>(pb, p.H, blk.ci > 0);
    else
      pair_bins_reduce_kernel<3><<<pb.nb * pb.nsh, PB_RTHREADS, (size_t)3 * 2 * pb.rf * p.H * sizeof(double), c->stream>>>(pb, p.H, blk.ci > 0);
    HIP_TRY(hipGetLastError());
    made_bins_clean(c);
    DBG_SYNC(c, "pair bins reduce");
  }
  // a skipped level must have found its input list empty (census_lists_kernel / tail_kernel check)
  fl.skipped = skip_mask(ep.need) & ~(fl.served3 ? 4 : 0);
  return 0;
}

// ---- the sums of the scattered moments are complete: mirror / diagonals / column sums, with the accumulator tail riding
// in the launch where it can
static int stats_finish(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, StatsFlow &fl) {
  const AccLayout &a = p.a;
  const i64 N = p.N;
  const int H = p.H, D = p.D;
  const bool masked = p.masked;
  SpanGuard g(c, KID_MISC);
  if (c->model == EVOAMD_MODEL_BSC) {
    TailArgs ta = {};  // (as for ES3C below) + a copy of Wq where the device update's inverse wants it
    if (p.nchunks == 1 && !masked && !c->reduce_pending) {
      ta = make_tail_args(c, a, N, false, fl.skipped);
      fl.tail_done = true;
    }
    double *wq_copy = (!c->comm && !masked && c->tmpA) ? c->tmpA : nullptr;
    made_wq_copy(c, wq_copy != nullptr);
    const unsigned fgrid = cdiv((i64)H * H, 256) + (fl.tail_done ? 1 : 0);
    if (p.bsc_wave)
      bsc_finish_kernel<<<fgrid, 256, 0, c->stream>>>(c->acc + a.Wq, c->acc + a.pies, c->acc_base + 4, BSC_CS_SLICES, H,
                                                       c->partial2, fl.bsc_grid, c->acc + a.sigma, fl.bsc_pb, ta, wq_copy);
    else
      bsc_finish_kernel<<<fgrid, 256, 0, c->stream>>>(c->acc + a.Wq, c->acc + a.pies, c->colpart, p.nblk, H, c->partial2,
                                                       cdiv(N, 4), c->acc + a.sigma, PairBins{}, ta, wq_copy);
  } else {
    const SsscArgs &sa = ep.sa;
    const i64 nthr = (i64)H * H > D ? (i64)H * H : D;
    // the accumulator tail (counters, census, list checks) as one more workgroup of this launch: one block of
    // datapoints, complete data, no fused E-step reduction pending (that one writes the scalars the tail reads)
    TailArgs ta = {};
    if (p.nchunks == 1 && !masked && !c->reduce_pending) {
      ta = make_tail_args(c, a, N, p.census, fl.skipped);
      fl.tail_done = true;
    }
    // complete data: the kernels left the column sums in CS_SLICES slices; else per-block partials of the rows
    if (p.kappa)  // the Lam terms of the diagonal second moments, into slice 0 of the column sums the launch below adds up
      sssc_finish_kernel<<<H, 256, 0, c->stream>>>(c->acc + a.xss, c->acc + a.xszsz, c->acc + a.xs, c->acc + a.xsz, sa.cs, CS_SLICES,
                                                   H, c->y2sum, c->acc + a.y2, D, sa.xss_o, sa.xszsz_o, c->PT, fl.pb, TailArgs{}, 2,
                                                   c->err, c->D1, sa.cs, sa.cs1);
    sssc_finish_kernel<<<cdiv(nthr, 256) + (fl.tail_done ? 1 : 0), 256, 0, c->stream>>>(
        c->acc + a.xss, c->acc + a.xszsz, c->acc + a.xs, c->acc + a.xsz, masked ? c->colpart : sa.cs,
        masked ? p.nblk : CS_SLICES, H, c->y2sum, c->acc + a.y2, D, sa.xss_o, sa.xszsz_o, masked ? nullptr : c->PT, fl.pb, ta,
        p.kappa ? 1 : 0, c->err);
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "colsum + finish");
  return 0;
}

// ---- one block's part of the K = N contraction (on stream2 where the pass has a second stream)
static int stats_contract_block(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep, const StatsBlock &blk, const StatsFlow &fl,
                                const double *Ywp, int ldwp) {
  const AccLayout &a = p.a;
  const i64 n0 = blk.n0, nc = blk.nc;
  const int H = p.H, D = p.D, ci = blk.ci;
  GemmTnOpts o;
  if (p.second_stream) {
    if (!fl.early_recorded) HIP_TRY(hipEventRecord(c->ev_chunk[ci], c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_chunk[ci], 0));
    // beside the Theta-update chain: leave slots per XCD to the chain's kernels (option "sk_spare", else the plan's)
    o.stream = c->stream2;
    o.spare = c->sk_spare >= 0 ? c->sk_spare : p.gemm_spare;
  }
  o.c_is_zero = true;  // acc was cleared at the top of stats_compute
  o.accumulate = p.nchunks > 1;
  o.mirror = ci == p.nchunks - 1;
  if (c->model == EVOAMD_MODEL_BSC && c->f32)
    return launch_gemm_tn_f32(c, c->Esf + (size_t)n0 * H, H, c->Yf + (size_t)n0 * D, D, c->acc + a.Wp, D, H, D, nc, o);
  if (c->model == EVOAMD_MODEL_BSC)  // Wp = Es^T Y  (H,D)
    return launch_gemm_tn(c, c->Es + (size_t)n0 * H, H, Ywp + (size_t)n0 * ldwp, ldwp, c->acc + a.Wp, D, H, D, nc, o);
  // [Y | Es | Ez]^T Ez  ->  Wp (D,H) | sum_n xpt_s (x) xpt_sz (H,H) | sum_n xpt_sz (x) xpt_sz (H,H)
  // (the last block is Ez^T Ez: symmetric, upper tiles only when its first row is tile-aligned;
  // launch_gemm_tn drops the hint if its tile does not divide it)
  o.sym_row0 = ((D + H) % GEMM_BM) == 0 ? D + H : -1;
  return launch_gemm_tn(c, c->Y + (size_t)n0 * c->ldY, c->ldY, ep.Ez + (size_t)n0 * c->ldY, c->ldY, c->acc + a.sWp, H,
                        D + 2 * H, H, nc, o);
}

// ---- ES3C on incomplete data: y_hat = Ez W^T with the Theta of this E-step: the reconstruction (sssc.py:613-627), the
// rows the Wp contraction reads (:631) and, squared over the reliable entries, the trace term of sigma2 (:640-645,751);
// then the two products from the reconstructed rows
static int stats_sssc_masked_products(evoamd_ctx *c, const StatsPlan &p, const Es3cPass &ep) {
  const AccLayout &a = p.a;
  const int H = p.H, D = p.D;
  TRY(reconstruct_rows(c, "ES3C on incomplete data needs do_reconstruction in every step (sssc.py:630-633)"));
  GemmTnOpts o;
  o.c_is_zero = true;
  o.sym_row0 = (H % GEMM_BM) == 0 ? H : -1;
  TRY(launch_gemm_tn(c, ep.Es, c->ldY, ep.Ez, c->ldY, c->acc + a.sWp + (size_t)D * H, H, 2 * H, H, p.N, o));
  o.sym_row0 = -1;
  return launch_gemm_tn(c, c->Yrec, D, ep.Ez, c->ldY, c->acc + a.sWp, H, D, H, p.N, o);
}

// ---- the second stream joins (or the caller will), the fused E-step's reduction, the accumulator tail where it did not
// ride in the finish launch, the all-reduce
static int stats_epilogue(evoamd_ctx *c, const StatsPlan &p, const StatsFlow &fl) {
  const AccLayout &a = p.a;
  const i64 N = p.N;
  if (p.second_stream) {
    HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
    if (p.fork_gemm)
      c->gemm_forked = true;  // the caller joins (after the H x H inverses)
    else
      HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  TRY(flush_reduce(c));  // fused E-step: free-energy term and counters into the scalar block (beside the forked contraction)
  {
    SpanGuard g(c, KID_MISC);
    if (!fl.tail_done) tail_kernel<<<1, 256, 0, c->stream>>>(make_tail_args(c, a, N, p.census, fl.skipped));
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "stats contraction + tail");
    made_clean_lists(c);
    if (c->model == EVOAMD_MODEL_SSSC && c->mask_infr) {  // tail[7] = sum over reliable entries of y_hat^2
      masked_sqsum_kernel<<<256, 256, 0, c->stream>>>(c->yhat, c->mask_infr, N * (i64)p.D, c->acc + a.tail + 7);
      HIP_TRY(hipGetLastError());
    }
    if (c->model == EVOAMD_MODEL_BSC && c->mask_infr && c->keep_differs) {
      // the keep-mask drops reliable entries: the reference's sigma reads y_reconstructed there (bsc.py:187,214-216), the
      // kernels' sum came from the lpj, i.e. from the data (with x == x_infr the two agree and nothing is launched)
      if (!c->yhat_valid) TRY(compute_reconstruction(c));
      bsc_sigma_rec_kernel<<<256, 256, 0, c->stream>>>(c->Y, c->ldY, c->Yrec, c->yhat, c->mask_infr, N, p.D, c->acc + a.sigma);
      HIP_TRY(hipGetLastError());
    }
  }
  if (c->comm && c->gemm_forked) {
    // [xs | xss | xsz | xszsz] and [y2 | tail] now; [Wp | s_sz | sz_sz] when the contraction has joined
    SpanGuard g(c, KID_ALLREDUCE);
    RCCL_TRY(g_rccl.AllReduce(c->acc, c->acc, (size_t)a.sWp, /*ncclDouble*/ 8, /*ncclSum*/ 0, c->comm, c->stream));
    RCCL_TRY(g_rccl.AllReduce(c->acc + a.y2, c->acc + a.y2, (size_t)(c->acc_n - a.y2), 8, 0, c->comm, c->stream));
    c->ar_gemm_pending = true;
  } else if (c->comm) {
    SpanGuard g(c, KID_ALLREDUCE);
    RCCL_TRY(g_rccl.AllReduce(c->acc, c->acc, (size_t)c->acc_n, /*ncclDouble*/ 8, /*ncclSum*/ 0, c->comm, c->stream));
  }
  return 0;
}

// ES3C: the argument block of the scatter kernels, the levels the final K^n needs, fresh on-the-fly lists
static int stats_sssc_pass(evoamd_ctx *c, const StatsPlan &p, Es3cPass &ep) {
  const AccLayout &a = p.a;
  const i64 N = p.N;
  const int H = p.H, D = p.D;
  ep.Es = c->model == EVOAMD_MODEL_SSSC ? c->Y + D : c->Es;
  ep.Ez = c->Y + D + H;
  ep.Ed = c->Y + D + 2 * H;
  if (c->model != EVOAMD_MODEL_SSSC) return 0;
  SsscArgs &sa = ep.sa;
  Batch b = {c->states, nullptr, c->Y, c->Bm, c->yy, N, c->S, 0, nullptr, c->L, c->S_perm, c->flags, KID_STATS, 0};
  b.mask = c->mask_infr;
  sa = sssc_args(c, b);
  sa.lpj_in = c->lpj;
  sa.rowmax = c->rowmax;
  sa.rowsum = c->rowsum;
  sa.Es = ep.Es;
  sa.Ez = ep.Ez;
  sa.Ed = ep.Ed;
  sa.ldE = c->ldY;
  sa.xss = c->acc + a.xss;
  sa.xszsz = c->acc + a.xszsz;
  sa.xss_o = c->acc_base + c->pre_n;
  sa.xszsz_o = c->acc_base + c->pre_n + (size_t)H * H;
  if (!p.masked) sa.cs = c->acc_base + 4;  // the kernels sum the columns of [Es | Ez] and the diagonal second moments themselves
  sa.cs1 = c->acc_base + 4 + (size_t)CS_SLICES * 3 * H;
  if (p.kappa) sa.kap_in = c->kap;
  ep.ls = es3c_lists(c, (int)list_cap(N * (i64)c->S));
  // the final K^n is made of resident states and accepted candidates: same levels as the candidates
  levels_for(c, p.lv, ep.need);
  return zero_lists(c);
}

// Everything of evoamd_stats up to (and including) the all-reduce; the packed accumulator stays on
// the device.  tail[7] receives ljc of the Theta the E-step ran with.
// fork_gemm: the caller promises to call join_fork before it reads the contraction's block of acc
// (evoamd_mstep_device: after the H x H inverses).  With a communicator (ES3C) the packed accumulator is
// all-reduced in two pieces: everything the inverses read here, the contraction's block at the join --
// all RCCL calls stay on the main stream, in the same order on every rank.  Not while kernels are being
// timed on the main stream.
static int stats_compute(evoamd_ctx *c, bool fork_gemm = false) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "configure, upload_data and set_params first");
  REQUIRE_KN(c);
  StatsPlan p;
  TRY(stats_plan(c, fork_gemm, p));
  // ---- preamble
  TRY(join_fork(c));  // a previous call that failed between fork and join must not race with the memset below
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure_bins_capacity(c));
  if (c->bins_dirty && c->pbins.gcnt)  // an earlier pass returned between its producers and the reduce: stale region counts
    HIP_TRY(hipMemsetAsync(c->pbins.gcnt, 0, (size_t)c->pbins.nb * c->pbins.nwg * sizeof(int), c->stream));
  // test hook: consumed by every pass (it stops only an ES3C pass on complete data, after its main kernel)
  const bool debug_fail = c->debug_fail_stats != 0;
  c->debug_fail_stats = 0;
  if (!c->acc_clean)  // (else: zeroed by the selection kernel on its way)
    HIP_TRY(hipMemsetAsync(c->acc_base, 0, (size_t)(c->ovf_n + c->acc_n) * sizeof(double), c->stream));
  on_stats_pass_begun(c);
  TRY(ensure_B(c));
  if (!c->rows_fresh) {  // otherwise vary_kn left rowmax / rowsum / dpar[DP_FS] behind
    TRY(row_lse(c, c->lpj, p.N, c->L, c->rowmax, c->rowsum, c->dpar + DP_FS));
  }
  StatsFlow fl;
  // the whole statistics pass (everything that reads K^n + lpj and leaves the M-step sums, the GEMM aside)
  std::unique_ptr<SpanGuard> pass(new SpanGuard(c, KID_STATS_PASS));
  TRY(c->colpart.ensure(c, (size_t)p.nblk * (c->model == EVOAMD_MODEL_BSC ? p.H : 3 * p.H)));
  Es3cPass ep;
  TRY(stats_sssc_pass(c, p, ep));
  const double *Ywp = c->Y;  // EBSC: what the Wp contraction reads
  int ldwp = c->ldY;
  if (c->model == EVOAMD_MODEL_SSSC && !p.masked && stats_bins_pay(c)) fl.pb = c->pbins;
  if (p.kappa) fl.pb.planes = 4;  // the pair states' q apart from the Lam-complete entries of the quad levels
  // ---- the blocks of datapoints
  for (int ci = 0; ci < p.nchunks; ci++) {
    const i64 n0 = (i64)ci * p.rows_per_chunk;
    const i64 nc = std::min<i64>(p.rows_per_chunk, p.N - n0);
    const StatsBlock blk = {ci, n0, nc, (int)(n0 / p.rpb), (int)cdiv(nc, p.rpb)};
    TRY(c->model == EVOAMD_MODEL_BSC ? stats_bsc_block(c, p, blk, fl, Ywp, ldwp)
        : p.masked                   ? stats_sssc_masked_block(c, p, ep)
                                     : stats_sssc_block(c, p, ep, blk, fl, debug_fail));
    if (ci == p.nchunks - 1) {
      // (before this block's contraction is enqueued: on one stream the span of the statistics pass must not cover it)
      TRY(stats_finish(c, p, ep, fl));
      pass.reset();
    }
    if (c->model == EVOAMD_MODEL_SSSC && p.masked) continue;  // two products from the reconstructed rows, below
    TRY(stats_contract_block(c, p, ep, blk, fl, Ywp, ldwp));
  }
  // ---- epilogue
  if (c->model == EVOAMD_MODEL_SSSC && p.masked) TRY(stats_sssc_masked_products(c, p, ep));
  TRY(stats_epilogue(c, p, fl));
  made_stats_rows(c);
  return 0;
}

extern "C" int evoamd_stats(evoamd_ctx *c, double *acc_out) {
  REQUIRE(acc_out, "acc_out is NULL");
  TRY(stats_compute(c));
  HIP_TRY(hipMemcpyAsync(c->h_acc, c->acc, ((size_t)c->acc_n + DP_COUNT) * sizeof(double), hipMemcpyDeviceToHost,
                         c->stream));
  const int r = check_err(c);  // synchronises the stream
  if (c->sssc_prec32 && c->model == EVOAMD_MODEL_SSSC) {
    // precision = float32: the reference keeps these sums in float32 arrays (sssc.py:484-498); here they are summed in
    // double and rounded once -- closer to the exact sums than the reference's own float32 running sums
    const AccLayout a = acc_layout(c);
    for (i64 i = 0; i < a.sWp; i++) c->h_acc[i] = (double)(float)c->h_acc[i];
    for (i64 i = a.s_sz; i < a.y2; i++) c->h_acc[i] = (double)(float)c->h_acc[i];
  }
  memcpy(acc_out, c->h_acc, (size_t)c->acc_n * sizeof(double));
  if (!r) made_level_hints(c, c->h_acc + c->acc_n);
  return r;
}

// ---------------------------------------------------------------------------------------
// device-side Theta update
// ---------------------------------------------------------------------------------------
// Inverts A (and B, if not null) in place; the two are independent.
static int launch_inverse_pivoted(evoamd_ctx *c, double *A, double *B, int n) {
  if (n <= GJR_N) {
    gj_inverse_reg_kernel<<<B ? 2 : 1, MS_T, 0, c->stream>>>(A, B, n, c->dpar + DP_STATUS);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  double *mats[2] = {A, B};
  const dim3 ugrid(cdiv(n, 64), cdiv(n, 64));
  if (n <= 1024) {  // blocked: register panel + fused interchange / rank-NB MFMA update, both matrices per launch
    const int nmat = B ? 2 : 1;
    GjMats gm;
    gm.a[0] = A;
    gm.a[1] = B ? B : A;
    gm.w[0] = c->gjwork;
    gm.w[1] = c->gjwork + (size_t)n * n;
    double *Dp = c->gjwork + (size_t)2 * n * n;  // 2 x n x NB (NB <= 32)
    double *Pn = Dp + (size_t)64 * n;
    int *ipiv = (int *)(Pn + (size_t)64 * n);
    int *perm = ipiv + 2 * n;
    const int rpt = n <= 256 ? 1 : 2;  // rows per thread of the panel kernel
    const int pthreads = cdiv(cdiv(n, rpt), 64) * 64;
    const dim3 ug(cdiv(n, 64), cdiv(n, 64), nmat);
    int flip = 0;
    for (int p0 = 0; p0 < n; p0 += 16, flip ^= 1) {
      const int pf = flip | (p0 ? 0 : 4);
      if (rpt == 1)
        gjp_panel_kernel<16, 1><<<nmat, pthreads, 0, c->stream>>>(gm, n, p0, pf, ipiv, perm, Pn, Dp, c->dpar + DP_STATUS);
      else
        gjp_panel_kernel<16, 2><<<nmat, pthreads, 0, c->stream>>>(gm, n, p0, pf, ipiv, perm, Pn, Dp, c->dpar + DP_STATUS);
      gjp_update_kernel<16><<<ug, 256, 0, c->stream>>>(gm, n, p0, flip, ipiv, Dp, Pn);
    }
    gjp_unscramble_kernel<<<dim3(n, nmat), 256, 0, c->stream>>>(gm, n, flip, perm);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  for (int m = 0; m < 2; m++) {
    if (!mats[m]) continue;
    for (int p = 0; p < n; p++) {
      gj_pivot_kernel<<<1, MS_T, 0, c->stream>>>(mats[m], n, p, c->gjwork, c->dpar + DP_STATUS);
      gj_update_kernel<<<ugrid, 256, 0, c->stream>>>(mats[m], n, p, c->gjwork);
    }
    gj_unscramble_kernel<<<n, 256, (size_t)n * (sizeof(double) + sizeof(int)), c->stream>>>(mats[m], n, c->gjwork);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// SPD block Gauss-Jordan (kernels_mstep.hpp: gjs_*): one launch per 16 columns, both matrices together.
static int launch_inverse_spd(evoamd_ctx *c, double *A, double *B, int n) {
  const int nmat = B ? 2 : 1;
  GjMats gm;
  gm.a[0] = A;
  gm.a[1] = B ? B : A;
  gm.w[0] = c->gjwork;
  gm.w[1] = c->gjwork + (size_t)n * n;
  double *Pinv = c->gjwork + (size_t)2 * n * n + (size_t)130 * n + 8;
  double *d0 = Pinv + 2 * 2 * GJS_B * GJS_B;
  // n <= 128: one launch, the matrix in the registers of one workgroup per matrix ("inverse_block" = 16 / 32 force the
  // multi-launch forms)
  if (n <= GJR_MAXN && c->spd_block == 0) {
    gjs_resident_kernel<<<nmat, 1024, 0, c->stream>>>(gm, n, c->dpar + DP_STATUS);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  // measured per inverse pair (tools/bench_inverse.py): n = 128 71 vs 73 us, 256 129 vs 141, 512 241 vs 286,
  // 1024 629 vs 774 -- the wider step pays from n = 256 on ("inverse_block" = 32 forces it from n = 32 for the tests)
  if (n >= GJS32 && (c->spd_block == 32 || (c->spd_block == 0 && n >= 256))) {
    double *Pinv32 = c->gjwork + (size_t)2 * n * n + (size_t)132 * n + 1040;
    gjs32_first_kernel<<<nmat, 64, 0, c->stream>>>(gm, n, Pinv32, d0, c->dpar + DP_STATUS);
    const dim3 grid32(cdiv(n, 64), cdiv(n, 64), nmat);
    int flip32 = 0;
    for (int p0 = 0; p0 < n; p0 += GJS32, flip32 ^= 1)
      gjs32_step_kernel<<<grid32, 256, 0, c->stream>>>(gm, n, p0, flip32, Pinv32, d0, c->dpar + DP_STATUS);
    HIP_TRY(hipGetLastError());
    if (flip32) {
      for (int k = 0; k < nmat; k++)
        HIP_TRY(hipMemcpyAsync(gm.a[k], gm.w[k], (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
  }
  gjs_first_kernel<<<nmat, 64, 0, c->stream>>>(gm, n, Pinv, d0, c->dpar + DP_STATUS);
  const dim3 grid(cdiv(n, 64), cdiv(n, 64), nmat);
  int flip = 0;
  for (int p0 = 0; p0 < n; p0 += GJS_B, flip ^= 1)
    gjs_step_kernel<<<grid, 256, 0, c->stream>>>(gm, n, p0, flip, Pinv, d0, c->dpar + DP_STATUS);
  HIP_TRY(hipGetLastError());
  if (flip) {  // odd number of block steps: the result sits in the partner buffers
    for (int k = 0; k < nmat; k++)
      HIP_TRY(hipMemcpyAsync(gm.a[k], gm.w[k], (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  return 0;
}

// force_pivot: the caller saw status == 3 from the SPD path and repeats the solve
static int launch_inverse(evoamd_ctx *c, double *A, double *B, int n, bool force_pivot = false) {
  if (c->spd_inverse && !force_pivot) return launch_inverse_spd(c, A, B, n);
  return launch_inverse_pivoted(c, A, B, n);
}

// ---- evoamd_mstep_device: what one call decides before it enqueues anything (mstep_plan); the stages only read it.
// learn_mask as include/evo_amd.h documents it: the five learn bits (L_W ... L_PSI, kernels_mstep.hpp) and two requests
enum : int {
  MSTEP_LEARN_BITS = L_W | L_PIES | L_MUS | L_SIGMA2 | L_PSI,
  MSTEP_WANT_REC = 32,    // also form the data estimate under the OLD Theta (evoamd_reconstruct)
  MSTEP_THETA_HOME = 64,  // Theta^new stays on the device: the caller fetches it on demand (evoamd_get_params_*, lazy Theta)
};

// lazy Theta: the host has no copy of the parameters the E-step ran with, and the update overwrites them in place; a copy
// is kept until the update is known to be well posed (evoamd_restore_theta_backup)
enum BackupRoute {
  BACKUP_NONE,
  BACKUP_IN_UPDATE,    // the first kernel of the ES3C update writes the copy on its way (backup_rides_in_update)
  BACKUP_SIDE_KERNEL,  // theta_backup_kernel on the side stream, beside the statistics pass; the update waits for ev_bak
};

// how the mailbox (sequence number, error words, accumulator tail, scalar block, Theta^new or not) reaches the host
enum PublishRoute {
  PUBLISH_FOLDED,       // the last kernel of the update writes the header: no mailbox kernel
  PUBLISH_MAIN,         // mailbox kernel on the main stream
  PUBLISH_SIDE,         // mailbox kernel on the side stream, beside derive_from_theta and the prefetched pass
  PUBLISH_COPY_ENGINE,  // Theta^new through the copy engine, a header-only mailbox kernel on the main stream
};

struct MstepPlan {
  int learn;         // the learn bits; 0 = statistics only
  bool want_rec;
  bool theta_home;
  bool force_pivot;  // the SPD retry: the H x H systems by the partially pivoted elimination
  BackupRoute backup;
  PublishRoute publish;
  bool theta_in_mailbox;  // the mailbox kernel carries W (| Psi | mus | pies) behind the header
};

// ES3C with D <= 8 H: the first kernel of the update (sssc_mstep_prepare_kernel, an H x H grid) writes the backup on its
// way, no launch and no event of its own.
static bool backup_rides_in_update(const evoamd_ctx *c) {
  return c->model == EVOAMD_MODEL_SSSC && c->D <= 8 * c->H;
}

// Routes of one call (learn = learn bits set, home = MSTEP_THETA_HOME, flops = contraction_flops, side = option
// "mailbox_side_stream", dma = option "theta_copy_engine"):
//
//   learn  home | backup                                   | Theta^new to the host     | header written by
//   -----------------------------------------------------------------------------------------------------------------
//   no     any  | none                                     | --                        | mailbox kernel (*)
//   yes    yes  | in the update (ES3C, D <= 8 H), else own | -- (fetched on demand)    | side && flops >= 8e9: mailbox
//               | kernel on the side stream                |                           | kernel, side stream; else the
//               |                                          |                           | update's last kernel (folded)
//   yes    no   | none                                     | dma: copy engine          | mailbox kernel, main stream
//               |                                          | else: the mailbox kernel  | mailbox kernel (**)
//
//   (*)  side stream when side && flops >= 8e9, else main stream      (**) the same with 8e10
//
// The SPD retry (status 3 from the first attempt) is the same plan with force_pivot, no backup (the first attempt took
// it, and Theta is half overwritten by now) and never folded.
//
// The mailbox kernel writes to pinned host memory and ends in a system-scope fence: 26 us of which nothing behind it in
// the stream depends.  On the side stream it runs beside derive_from_theta / the prefetched pass; what it reads (tail,
// scalar block, error words, Theta) is next written by the NEXT iteration's kernels, which the host enqueues only after
// it has seen this mailbox.  Measured, ms per iteration lazy / eager Theta: c4 3.94 -> 3.88 / 4.43 -> 4.05, N / 8 shard
// 1.13 -> 1.08 / 1.37 -> 1.60, c2 0.386 -> 0.404: the event pair costs ~10 us, and a 3 MB Theta copy beside the refresh
// only delays the host -- so only the mailbox of a long iteration goes there, with Theta on board only at the north-star
// size.  Folding needs the mailbox on the main stream and nothing but the header in it.
// Enqueues nothing and changes nothing in the context.
static MstepPlan mstep_plan(const evoamd_ctx *c, int learn_mask, bool spd_retry) {
  MstepPlan p = {};
  p.learn = learn_mask & MSTEP_LEARN_BITS;
  p.want_rec = (learn_mask & MSTEP_WANT_REC) != 0;
  p.theta_home = (learn_mask & MSTEP_THETA_HOME) != 0;
  p.force_pivot = spd_retry;
  p.backup = BACKUP_NONE;
  if (p.learn && p.theta_home && !spd_retry) p.backup = backup_rides_in_update(c) ? BACKUP_IN_UPDATE : BACKUP_SIDE_KERNEL;
  const bool theta_out = p.learn && !p.theta_home;  // Theta^new goes to the host with this call
  if (theta_out && c->theta_copy_engine) {
    p.publish = PUBLISH_COPY_ENGINE;
    return p;
  }
  p.theta_in_mailbox = theta_out;
  if (c->mbox_side && contraction_flops(c) >= (theta_out ? 8e10 : 8e9))
    p.publish = PUBLISH_SIDE;
  else
    p.publish = (p.learn && p.theta_home && !spd_retry) ? PUBLISH_FOLDED : PUBLISH_MAIN;
  return p;
}

// Theta^new from the device accumulator (which stats_compute left behind) and the clamps; all stream-ordered, no host
// arithmetic.  What only the NEXT E-step reads is derive_from_theta's, which evoamd_mstep_device enqueues behind the
// mailbox: the host gets F and Theta^new one GEMM earlier and is ahead of the stream again by the time that finishes.
// Both end in the one scalar kernel that writes the mailbox header on its way when fold_seq != 0 (PUBLISH_FOLDED).
static int theta_update_sssc(evoamd_ctx *c, const MstepPlan &p, unsigned long long fold_seq) {
  const AccLayout a = acc_layout(c);
  const int H = c->H, D = c->D, learn = p.learn;
  const i64 HH = (i64)H * H;
  const double *Nptr = c->acc + a.tail + 3;
  double *bak = p.backup == BACKUP_IN_UPDATE ? c->theta_bak : nullptr;
  int r = 0;
  if (c->sssc_prec32)  // precision = float32: the moment sums as float32 values (evoamd_stats does the same on the host)
    round_f32_kernel<<<cdiv(a.sWp, 256), 256, 0, c->stream>>>(c->acc, a.sWp);
  // mus / pies first (Psi needs the NEW mus, sssc.py:733), then both H x H inverses in one launch:
  // tmpA <- xpt_szsz (for W, sssc.py:693), tmpB <- xpt_ss + eps I (for Psi, sssc.py:738)
  sssc_mstep_prepare_kernel<<<cdiv(HH, 256), 256, 0, c->stream>>>(c->acc + a.xs, c->acc + a.xsz, c->acc + a.xss,
                                                                  c->acc + a.xszsz, Nptr, H, learn,
                                                                  c->pies, c->mus, c->tmpA, c->tmpC, c->tmpB, bak, c->W,
                                                                  c->Psi, c->dpar, D, c->bg_unit);
  if ((learn & L_W) && (learn & L_PSI))
    r = launch_inverse(c, c->tmpA, c->tmpB, H, p.force_pivot);
  else if (learn & L_W)
    r = launch_inverse(c, c->tmpA, nullptr, H, p.force_pivot);
  else if (learn & L_PSI)
    r = launch_inverse(c, c->tmpB, nullptr, H, p.force_pivot);
  if (r) return r;
  TRY(join_fork(c));  // sWp / s_sz / sz_sz come from the contraction
  if (c->sssc_prec32) round_f32_kernel<<<cdiv(a.y2 - a.s_sz, 256), 256, 0, c->stream>>>(c->acc + a.s_sz, a.y2 - a.s_sz);
  if (learn & L_W)
    launch_gemm_nn_raw(c, c->acc + a.sWp, H, c->tmpA, H, c->W, H, D, H, H);
  const bool masked = c->mask_infr != nullptr;  // sssc.py:747-755: the trace term arrives in tail[7]
  // (Psi's element-wise finish rides along with the trace partials below when both run)
  const bool psi_with_trace = (learn & L_PSI) && (learn & L_SIGMA2) && !masked;
  if ((learn & L_PSI) && !psi_with_trace)
    sssc_psi_finish_kernel<<<cdiv(HH, 256), 256, 0, c->stream>>>(c->tmpC, c->tmpB, c->acc + a.s_sz, c->mus, H, c->Psi);
  else if (!(learn & L_PSI))
    psi_floor_kernel<<<cdiv(H, 256), 256, 0, c->stream>>>(c->Psi, H);
  HIP_TRY(hipGetLastError());
  GemmTnOpts gram;
  gram.deterministic = true;
  TRY(launch_gemm_tn(c, c->W, H, c->W, H, c->G, H, H, H, D, gram));  // G = W^T W (new W)
  const int n_part = (int)std::min<i64>(1024, cdiv(HH, 1024));
  TRY(c->colpart.ensure(c, (size_t)n_part));
  if (psi_with_trace)
    sssc_trace_partial_kernel<<<n_part, 256, 0, c->stream>>>(c->acc + a.sz_sz, c->G, H, cdiv(HH, n_part), c->colpart, c->tmpC,
                                                             c->tmpB, c->acc + a.s_sz, c->mus, c->Psi);
  else if ((learn & L_SIGMA2) && !masked)
    sssc_trace_partial_kernel<<<n_part, 256, 0, c->stream>>>(c->acc + a.sz_sz, c->G, H, cdiv(HH, n_part), c->colpart);
  sssc_sigma_precompute_kernel<<<1, MS_T, 0, c->stream>>>(c->acc + a.y2, D, c->colpart, masked ? 0 : n_part, H, Nptr, learn,
                                                          c->pies, c->pilbar_v, c->dpar, masked ? c->rel_frac : -1.0,
                                                          c->acc + a.tail + 7, c->sssc_prec32,
                                                          fold_seq ? c->h_theta_dev : nullptr, c->acc + a.tail, c->err, fold_seq);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int theta_update_bsc(evoamd_ctx *c, const MstepPlan &p, unsigned long long fold_seq) {
  const AccLayout a = acc_layout(c);
  const int H = c->H, D = c->D, learn = p.learn;
  if (learn & L_W) {  // W^T = solve(Wq, Wp)  (bsc.py:237; lstsq == solve for a non-singular Wq)
    if (!c->wq_copy_valid || p.force_pivot)  // (else the finish kernel of the statistics pass left the copy in tmpA)
      HIP_TRY(hipMemcpyAsync(c->tmpA, c->acc + a.Wq, (size_t)H * H * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    made_wq_copy(c, false);
    TRY(launch_inverse(c, c->tmpA, nullptr, H, p.force_pivot));
    TRY(join_fork(c));  // Wp comes from the contraction
    if (!launch_gemm_nn_raw(c, c->tmpA, H, c->acc + a.Wp, D, c->Wt, D, H, D, H, c->W, H))  // W^T, and W on the way
      transpose_kernel<<<cdiv((i64)H * D, 256), 256, 0, c->stream>>>(c->Wt, H, D, c->W);
  }
  bsc_scalars_kernel<<<1, MS_T, 0, c->stream>>>(c->acc + a.pies, c->acc + a.sigma, H, D, c->acc + a.tail + 3, learn, c->dpar,
                                                c->mask_infr ? c->rel_frac : -1.0, fold_seq ? c->h_theta_dev : nullptr,
                                                c->acc + a.tail, c->err, fold_seq, c->bg_unit);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the update of the context's model; Theta on the device is Theta^new behind it (on_theta_updated: B = Y W is stale)
static int theta_update(evoamd_ctx *c, const MstepPlan &p, unsigned long long fold_seq) {
  on_theta_update_begun(c);
  SpanGuard g(c, KID_MSTEP);
  return c->model == EVOAMD_MODEL_SSSC ? theta_update_sssc(c, p, fold_seq) : theta_update_bsc(c, p, fold_seq);
}

// y_hat = E W^T with E = Es (EBSC) / Ez (ES3C) rows of the last statistics pass (see evoamd_reconstruct)
static int compute_reconstruction(evoamd_ctx *c) {
  REQUIRE(!c->f32, "reconstruction is not available in the float32 mode");
  const size_t need = (size_t)c->N * c->D;
  TRY(c->yhat.ensure(c, need));
  const double *Wt = c->Wt;
  const double *E = c->Es;
  int lde = c->H;
  if (c->model == EVOAMD_MODEL_SSSC) {
    if (!c->tmpWt) TRY(c->tmpWt.alloc((size_t)c->H * c->D));
    transpose_kernel<<<cdiv((i64)c->H * c->D, 256), 256, 0, c->stream>>>(c->W, c->D, c->H, c->tmpWt);  // (D,H) -> (H,D)
    Wt = c->tmpWt;
    E = c->Y + c->D + c->H;  // Ez block of [Y | Es | Ez | Ed]
    lde = c->ldY;
  }
  SpanGuard g(c, KID_GEMM);
  launch_gemm_nn_raw(c, E, lde, Wt, c->D, c->yhat, c->D, c->N, c->D, c->H);
  HIP_TRY(hipGetLastError());
  made_yhat(c);
  return 0;
}

extern "C" int evoamd_reconstruct(evoamd_ctx *c, double *y_hat) {
  REQUIRE(c && c->configured && c->have_data && c->have_params && y_hat, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->yhat_valid) {
    REQUIRE(c->stats_rows_valid, "evoamd_reconstruct: call evoamd_stats first (and before setting new parameters)");
    TRY(compute_reconstruction(c));
  }
  HIP_TRY(hipMemcpyAsync(y_hat, c->yhat, (size_t)c->N * c->D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Everything an EM iteration returns to the host goes through the mailbox; the host polls the sequence number.
struct MailboxTicket {
  unsigned long long seq;  // what the header will carry
  hipStream_t stream;      // the stream its writer is on: what the poll synchronises with when spinning takes too long
};

// Enqueues whatever p.publish asks for.  fold_seq: what the update's last kernel was given (PUBLISH_FOLDED).
static int mailbox_publish(evoamd_ctx *c, const MstepPlan &p, unsigned long long fold_seq, MailboxTicket &t) {
  t.stream = c->stream;
  if (p.publish == PUBLISH_FOLDED) {
    t.seq = fold_seq;
    return 0;
  }
  const AccLayout a = acc_layout(c);
  const size_t DH = (size_t)c->D * c->H, HH = (size_t)c->H * c->H, H = c->H;
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  if (p.publish == PUBLISH_COPY_ENGINE) {
    // Theta^new is final on the main stream here: the copy engine takes it from there, beside whatever follows
    double *dst = c->h_theta + MAILBOX_HDR;
    HIP_TRY(hipEventRecord(c->ev_theta, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream_copy, c->ev_theta, 0));
    HIP_TRY(hipMemcpyAsync(dst, c->W, DH * sizeof(double), hipMemcpyDeviceToHost, c->stream_copy));
    if (sssc) {
      HIP_TRY(hipMemcpyAsync(dst + DH, c->Psi, HH * sizeof(double), hipMemcpyDeviceToHost, c->stream_copy));
      HIP_TRY(hipMemcpyAsync(dst + DH + HH, c->mus, H * sizeof(double), hipMemcpyDeviceToHost, c->stream_copy));
      HIP_TRY(hipMemcpyAsync(dst + DH + HH + H, c->pies, H * sizeof(double), hipMemcpyDeviceToHost, c->stream_copy));
    }
    HIP_TRY(hipEventRecord(c->ev_theta_done, c->stream_copy));
  }
  MailboxSegs segs = {};
  if (p.theta_in_mailbox) {
    segs.src[0] = c->W;
    segs.n[0] = (long long)DH;
    if (sssc) {
      segs.src[1] = c->Psi;
      segs.n[1] = (long long)HH;
      segs.src[2] = c->mus;
      segs.n[2] = (long long)H;
      segs.src[3] = c->pies;
      segs.n[3] = (long long)H;
    }
  }
  t.seq = ++c->mbox_seq;
  const long long total = MAILBOX_HDR + (p.theta_in_mailbox ? (long long)(DH + HH + 2 * H) : 0);
  const int grid = (int)std::min<long long>(64, cdiv(total, 256 * 8));
  if (p.publish == PUBLISH_SIDE) {
    HIP_TRY(hipEventRecord(c->ev_mbox, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream_copy, c->ev_mbox, 0));
    t.stream = c->stream_copy;
  }
  mailbox_kernel<<<grid < 1 ? 1 : grid, 256, 0, t.stream>>>(c->h_theta_dev, c->acc + a.tail, c->err, segs, c->mbox_counter, t.seq);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The next iteration's pass over K^n, behind the mailbox in stream order: the host is released before it runs.
static void prefetch_next_pass(evoamd_ctx *c) {
  if (!c->prefetch_lpj || c->mask_infr || c->last_estep_fused) return;  // (a fused E-step evaluates K^n itself)
  // the host has not read this iteration's overflow counts yet (they arrive with the mailbox being polled next), so
  // res_need / res_cnt still describe the K^n of the PREVIOUS iteration: conservative levels
  drop_prefetch(c);
  if (lpj_resident_launch(c, c->lpj_alt, batch_hints(c, 0, /*prefetched=*/true)) == 0) made_prefetch(c);
}

// Spins on the sequence number (falls back to a blocking synchronise after 20 ms of spinning).
static int mailbox_poll(evoamd_ctx *c, const MstepPlan &p, const MailboxTicket &t) {
  volatile unsigned long long *flag = (volatile unsigned long long *)c->h_theta.get();
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (*flag != t.seq) {
    __builtin_ia32_pause();
    if ((++spins & 0xFFFu) == 0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02) {
      HIP_TRY(hipStreamSynchronize(t.stream));
      if (*flag != t.seq) return fail(EVOAMD_E_HIP, "mailbox kernel finished without publishing its sequence number");
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (p.publish == PUBLISH_COPY_ENGINE) HIP_TRY(hipEventSynchronize(c->ev_theta_done));
  return 0;
}

static int mailbox_errors(evoamd_ctx *c) {
  const int *e = (const int *)(c->h_theta + 1);
  if (e[0]) {
    HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int), c->stream));
    if (e[0] & 4) return fail(EVOAMD_E_INVALID, "internal: an ES3C overflow level was skipped although its list was not empty");
    if (e[0] & EVO_ERR_LIST_FULL) return fail(EVOAMD_E_INVALID, "internal: an ES3C overflow list was full, states were dropped");
    if (e[0] & EVO_ERR_BAD_ENTRY) return fail(EVOAMD_E_INVALID, "internal: an ES3C list entry or latent index read back from LDS was out of range");
    if (e[0] & 1) return fail(EVOAMD_E_KLIMIT, "ES3C: a state has more than %d active latents", SSSC_KCAP);
    return fail(EVOAMD_E_SINGULAR, "ES3C: exactly singular k x k system (the reference takes pinv here)");
  }
  return 0;
}

// Segments of the parameters on the device (W | Psi | mus | pies | scalar block) for theta_backup_kernel
static CopySegs theta_segs(evoamd_ctx *c) {
  CopySegs s = {};
  s.ptr[0] = c->W;
  s.n[0] = (long long)c->D * c->H;
  if (c->model == EVOAMD_MODEL_SSSC) {
    s.ptr[1] = c->Psi;
    s.n[1] = (long long)c->H * c->H;
    s.ptr[2] = c->mus;
    s.n[2] = c->H;
    s.ptr[3] = c->pies;
    s.n[3] = c->H;
  }
  s.ptr[4] = c->dpar;
  s.n[4] = DP_COUNT;
  return s;
}

// Room for the copy of Theta the plan asks for and, on the side-kernel route, the copy itself: on the side stream,
// beside the statistics pass (nothing writes Theta between the E-step and the update, which waits for ev_bak) -- one launch
// (3 MB at the north-star shape, ~3 us), 9 us that were in front of the update.  Before the statistics pass is enqueued.
static int mstep_backup(evoamd_ctx *c, const MstepPlan &p) {
  if (p.backup == BACKUP_NONE) return 0;
  const CopySegs s = theta_segs(c);
  size_t n = 0;
  for (int k = 0; k < 5; k++) n += (size_t)s.n[k];
  TRY(c->theta_bak.ensure(c, n));
  if (p.backup == BACKUP_IN_UPDATE) return 0;  // (valid once the update is enqueued: mstep_attempt)
  theta_backup_kernel<<<(unsigned)std::min<size_t>(256, cdiv((i64)n, 256 * 8)), 256, 0, c->stream_copy>>>(c->theta_bak, s, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev_bak, c->stream_copy));
  made_theta_backup(c);
  return 0;
}

extern "C" int evoamd_restore_theta_backup(evoamd_ctx *c) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(c->theta_bak && c->theta_bak_valid, "no parameter backup (evoamd_mstep_device keeps one when Theta stays on the device)");
  HIP_TRY(hipSetDevice(c->device));
  TRY(join_fork(c));
  HIP_TRY(hipStreamSynchronize(c->stream_copy));
  theta_backup_kernel<<<256, 256, 0, c->stream>>>(c->theta_bak, theta_segs(c), 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the raw parameters are back; everything derived from them (G, tables, B = Y W) is rebuilt by the next set_params
  on_theta_restored(c);
  return 0;
}

// One attempt at Theta^new and its way to the host.  Enqueued in this order: update, publish, what the next E-step
// derives from Theta^new, the prefetched pass; then the host polls.
static int mstep_attempt(evoamd_ctx *c, const MstepPlan &p) {
  unsigned long long fold_seq = 0;
  if (p.learn) {
    if (p.publish == PUBLISH_FOLDED) fold_seq = ++c->mbox_seq;
    TRY(theta_update(c, p, fold_seq));
    on_theta_updated(c, p.backup == BACKUP_IN_UPDATE);
  }
  TRY(join_fork(c));
  // accumulator tail (8) and the scalar block (16) are adjacent in device memory and in the mailbox;
  // the reference's step() hands Theta^new back, so it rides along unless it stays home
  MailboxTicket t;
  TRY(mailbox_publish(c, p, fold_seq, t));
  if (p.learn) {
    SpanGuard g(c, KID_MSTEP);
    TRY(derive_from_theta(c, /*updated=*/true));
  }
  prefetch_next_pass(c);
  return mailbox_poll(c, p, t);
}

// The mailbox has arrived: tail and scalar block to the caller, error words, overflow levels; after status 1 / 2 the
// clean-up that lets the caller finish the step on the host.
static int mstep_deliver(evoamd_ctx *c, const MstepPlan &p, double *tail_out, double *dpar_out) {
  const double *h = c->h_theta + 8;
  memcpy(tail_out, h, 8 * sizeof(double));
  memcpy(dpar_out, h + 8, DP_COUNT * sizeof(double));
  memcpy(c->h_dpar, h + 8, DP_COUNT * sizeof(double));
  TRY(mailbox_errors(c));
  made_level_hints(c, c->h_dpar);
  made_theta_mailbox(c, p.learn != 0 && !p.theta_home && c->h_dpar[DP_STATUS] == 0.0);
  if (c->h_dpar[DP_STATUS] == 0.0) return 0;
  dpar_out[DP_STATUS] = c->h_dpar[DP_STATUS];  // 1 singular, 2 non-finite: the caller may finish the step on the host
  HIP_TRY(hipMemsetAsync(c->dpar + DP_STATUS, 0, sizeof(double), c->stream));
  // derive_from_theta and the prefetched pass behind the mailbox ran with the failed update's Theta: drop the pass and
  // the clamp flags it may have raised (the caller re-installs a Theta before anything else is evaluated)
  on_theta_update_failed(c);
  HIP_TRY(hipMemsetAsync(c->flags, 0, (size_t)3 * c->N * sizeof(unsigned), c->stream));
  HIP_TRY(hipMemsetAsync(c->err, 0, 2 * sizeof(int), c->stream));
  return fail(EVOAMD_E_SINGULAR, "device Theta update: %s",
              c->h_dpar[DP_STATUS] == 1.0 ? "singular H x H system (the reference falls back to pinv / lstsq here)"
                                          : "non-finite sigma / pi");
}

extern "C" int evoamd_mstep_device(evoamd_ctx *c, int learn_mask, double *tail_out, double *dpar_out) {
  REQUIRE(tail_out && dpar_out, "NULL output");
  REQUIRE(!(c && c->mask_infr && c->rel_frac < 0.0), "incomplete data: evoamd_set_reliable_fraction first (bsc.py:113-118)");
  const MstepPlan p = mstep_plan(c, learn_mask, /*spd_retry=*/false);
  drop_theta_backup(c);
  TRY(mstep_backup(c, p));
  TRY(stats_compute(c, /*fork_gemm=*/true));
  made_theta_mailbox(c, false);
  if (p.want_rec && !c->yhat_valid) {  // under the Theta the E-step used, i.e. before the update
    TRY(compute_reconstruction(c));     // (incomplete data: the statistics pass formed it already)
  }
  if (p.backup == BACKUP_SIDE_KERNEL) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_bak, 0));
  TRY(mstep_attempt(c, p));
  if (p.learn && c->h_theta[8 + 8 + DP_STATUS] == 3.0) {
    // the SPD block elimination met a non-positive pivot: repeat the Theta update with partial
    // pivoting.  The statistics are still in acc; ljc moves back so that the update kernels shift
    // it into ljc_prev again.
    c->spd_fallbacks++;
    HIP_TRY(hipMemsetAsync(c->dpar + DP_STATUS, 0, sizeof(double), c->stream));
    HIP_TRY(hipMemcpyAsync(c->dpar + DP_LJC, c->dpar + DP_LJC_PREV, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    TRY(mstep_attempt(c, mstep_plan(c, learn_mask, /*spd_retry=*/true)));
  }
  return mstep_deliver(c, p, tail_out, dpar_out);
}

extern "C" int evoamd_gemm_tn(evoamd_ctx *c, const double *A, const double *B, double *C, int64_t K, int M, int Nc,
                              int sym_row0) {
  REQUIRE(c && A && B && C && K > 0 && M > 0 && Nc > 0, "bad arguments");
  REQUIRE(sym_row0 < 0 || (sym_row0 + Nc == M), "sym_row0: the symmetric block must be the last Nc rows of C");
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<double> dA, dB, dC;
  TRY(dA.alloc((size_t)K * M));
  TRY(dB.alloc((size_t)K * Nc));
  TRY(dC.alloc((size_t)M * Nc));
  int r = 0;
  hipError_t e = hipMemcpyAsync(dA, A, (size_t)K * M * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dB, B, (size_t)K * Nc * sizeof(double), hipMemcpyHostToDevice, c->stream);
  GemmTnOpts o;
  o.sym_row0 = sym_row0;
  if (e == hipSuccess) r = launch_gemm_tn(c, dA, M, dB, Nc, dC, Nc, M, Nc, K, o);
  if (e == hipSuccess && !r) e = hipMemcpyAsync(C, dC, (size_t)M * Nc * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(EVOAMD_E_HIP, "evoamd_gemm_tn: %s", hipGetErrorString(e));
  return r;
}

// One padded operand of evoamd_dense_probe on the device: `off` elements, guard rows, the logical rows, guard rows.
struct ProbeBuf {
  DevBuf<double> d;  // (16-byte aligned; holds floats as well)
  size_t bytes = 0;
  int up(const void *h, size_t off, size_t rows, size_t ld, int guard, size_t elem, hipStream_t s) {
    bytes = (off + (rows + 2 * (size_t)guard) * ld) * elem;
    TRY(d.alloc((bytes + 7) / 8));
    HIP_TRY(hipMemcpyAsync(d.get(), h, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  int down(void *h, hipStream_t s) const {
    HIP_TRY(hipMemcpyAsync(h, d.get(), bytes, hipMemcpyDeviceToHost, s));
    return 0;
  }
  template <typename T>
  T *base(size_t off, size_t ld, int guard) const {
    return (T *)d.get() + off + (size_t)guard * ld;
  }
};

extern "C" int evoamd_dense_probe(evoamd_ctx *c, const evoamd_dense_desc *d, const void *A, const void *B, const void *A2,
                                  void *C, void *side, evoamd_dense_route *route) {
  REQUIRE(c && d && A && C, "evoamd_dense_probe: bad arguments");
  const int op = d->op, M = d->M, Nc = d->Nc, g = d->guard;
  const i64 K = d->K;
  REQUIRE(op >= EVOAMD_DENSE_TN && op <= EVOAMD_DENSE_COLSUM_SQ, "evoamd_dense_probe: unknown op");
  REQUIRE(M > 0 && Nc > 0 && K > 0 && g >= 0 && d->off_a >= 0 && d->off_b >= 0 && d->off_c >= 0, "evoamd_dense_probe: bad shape");
  const bool colsum = op == EVOAMD_DENSE_COLSUM || op == EVOAMD_DENSE_COLSUM_SQ;
  const bool nn = op == EVOAMD_DENSE_NN;
  const bool f32 = op == EVOAMD_DENSE_TN_F32 || op == EVOAMD_DENSE_ROWS_F32;
  const bool same = d->same_operand != 0;
  const size_t ea = f32 ? sizeof(float) : sizeof(double);
  const size_t ec = op == EVOAMD_DENSE_ROWS_F32 ? sizeof(float) : sizeof(double);
  const i64 rowsA = nn ? M : K, colsA = nn ? K : M, rowsC = colsum ? 1 : M, colsC = colsum ? M : Nc;
  REQUIRE(d->lda >= colsA && d->ldc >= colsC && K <= INT32_MAX, "evoamd_dense_probe: a leading dimension is shorter than its row");
  REQUIRE(colsum || same || (B && d->ldb >= Nc), "evoamd_dense_probe: B");
  REQUIRE(!same || (op == EVOAMD_DENSE_TN && M == Nc), "evoamd_dense_probe: same_operand is the Gram route of op TN");
  REQUIRE(d->sym_row0 < 0 || (d->sym_row0 + Nc == M), "sym_row0: the symmetric block must be the last Nc rows of C");
  REQUIRE(op != EVOAMD_DENSE_ROWS_F32 || (A2 && d->lda2 >= K), "evoamd_dense_probe: ROWS_F32 needs the row-major A2");
  REQUIRE(!(nn && d->ldct > 0) || (side && d->ldct >= M), "evoamd_dense_probe: Ct");
  REQUIRE(!d->diag || (op == EVOAMD_DENSE_TN && side), "evoamd_dense_probe: diag");
  HIP_TRY(hipSetDevice(c->device));
  const hipStream_t s = c->stream;
  ProbeBuf bA, bB, bA2, bC, bS;
  TRY(bA.up(A, d->off_a, rowsA, d->lda, g, ea, s));
  if (!colsum && !same) TRY(bB.up(B, d->off_b, K, d->ldb, g, ea, s));
  if (op == EVOAMD_DENSE_ROWS_F32) TRY(bA2.up(A2, 0, M, d->lda2, g, ea, s));
  TRY(bC.up(C, d->off_c, rowsC, d->ldc, g, ec, s));
  const bool want_ct = nn && d->ldct > 0;
  if (want_ct) TRY(bS.up(side, 0, Nc, d->ldct, g, sizeof(double), s));
  if (d->diag) TRY(bS.up(side, 0, M, 1, g, sizeof(double), s));
  c->route = {};
  int r = 0;
  if (op == EVOAMD_DENSE_TN) {
    GemmTnOpts o;
    o.deterministic = d->deterministic != 0;
    o.sym_row0 = d->sym_row0;
    o.c_is_zero = d->c_is_zero != 0;
    o.accumulate = d->accumulate != 0;
    o.mirror = d->mirror != 0;
    o.spare = d->spare;
    o.diag = d->diag ? bS.base<double>(0, 1, g) : nullptr;
    const double *pa = bA.base<double>(d->off_a, d->lda, g);
    const double *pb = same ? pa : bB.base<double>(d->off_b, d->ldb, g);
    r = launch_gemm_tn(c, pa, d->lda, pb, same ? d->lda : d->ldb, bC.base<double>(d->off_c, d->ldc, g), d->ldc, M, Nc, K, o);
  } else if (op == EVOAMD_DENSE_TN_F32) {
    GemmTnOpts o;
    o.spare = d->spare;
    r = launch_gemm_tn_f32(c, bA.base<float>(d->off_a, d->lda, g), d->lda, bB.base<float>(d->off_b, d->ldb, g), d->ldb,
                           bC.base<double>(d->off_c, d->ldc, g), d->ldc, M, Nc, K, o);
  } else if (nn) {
    launch_gemm_nn_raw(c, bA.base<double>(d->off_a, d->lda, g), d->lda, bB.base<double>(d->off_b, d->ldb, g), d->ldb,
                       bC.base<double>(d->off_c, d->ldc, g), d->ldc, M, Nc, (int)K, want_ct ? bS.base<double>(0, d->ldct, g) : nullptr,
                       d->ldct);
  } else if (op == EVOAMD_DENSE_ROWS) {
    const double *pa = bA.base<double>(d->off_a, d->lda, g), *pb = bB.base<double>(d->off_b, d->ldb, g);
    REQUIRE(gemm_vec_ok(pa, d->lda) && gemm_vec_ok(pb, d->ldb) && (Nc % 2) == 0,
            "evoamd_dense_probe: ROWS reads 16-byte pieces (even ld, aligned bases, even Nc: what evoamd_configure grants)");
    launch_rows_f64(c, pa, d->lda, pb, d->ldb, bC.base<double>(d->off_c, d->ldc, g), d->ldc, M, Nc, K);
  } else if (op == EVOAMD_DENSE_ROWS_F32) {
    launch_rows_f32(c, bA.base<float>(d->off_a, d->lda, g), d->lda, bA2.base<float>(0, d->lda2, g), d->lda2,
                    bB.base<float>(d->off_b, d->ldb, g), d->ldb, bC.base<float>(d->off_c, d->ldc, g), d->ldc, M, Nc, (int)K);
  } else if (op == EVOAMD_DENSE_COLSUM) {
    launch_colsum<false>(c, bA.base<double>(d->off_a, d->lda, g), d->lda, K, M, bC.base<double>(d->off_c, d->ldc, g));
  } else {
    launch_colsum<true>(c, bA.base<double>(d->off_a, d->lda, g), d->lda, K, M, bC.base<double>(d->off_c, d->ldc, g));
  }
  if (r) return r;
  HIP_TRY(hipGetLastError());
  TRY(bC.down(C, s));
  if (want_ct || d->diag) TRY(bS.down(side, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (route) {
    *route = c->route;
    route->n_cu = c->n_cu;
  }
  return 0;
}

extern "C" int evoamd_inverse(evoamd_ctx *c, double *A, double *B, int n, double *timing_ms) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(A && n == c->H, "A must be H x H of the configured context");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)n * n * sizeof(double);
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  double st = 0.0;
  int r = 0;
  for (int attempt = 0; attempt < 2; attempt++) {  // second pass: pivoted repeat after an SPD failure
    HIP_TRY(hipMemcpyAsync(c->tmpA, A, bytes, hipMemcpyHostToDevice, c->stream));
    if (B) HIP_TRY(hipMemcpyAsync(c->tmpB, B, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->dpar + DP_STATUS, 0, sizeof(double), c->stream));
    HIP_TRY(hipEventRecord(e0, c->stream));
    r = launch_inverse(c, c->tmpA, B ? c->tmpB : nullptr, n, attempt == 1);
    HIP_TRY(hipEventRecord(e1, c->stream));
    if (r) break;
    HIP_TRY(hipMemcpyAsync(c->h_dpar + DP_COUNT, c->dpar + DP_STATUS, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->dpar + DP_STATUS, 0, sizeof(double), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st = c->h_dpar[DP_COUNT];
    if (st != 3.0) break;
    c->spd_fallbacks++;
  }
  float ms = 0.f;
  if (!r) {
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (st == 0.0) {
      HIP_TRY(hipMemcpyAsync(A, c->tmpA, bytes, hipMemcpyDeviceToHost, c->stream));
      if (B) HIP_TRY(hipMemcpyAsync(B, c->tmpB, bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (timing_ms) *timing_ms = ms;
  if (r) return r;
  if (st != 0.0) return fail(EVOAMD_E_SINGULAR, "evoamd_inverse: singular %d x %d system", n, n);
  return 0;
}

extern "C" int evoamd_get_params_bsc(evoamd_ctx *c, double *W, double *pi, double *sigma) {
  REQUIRE(c && c->configured && c->model == EVOAMD_MODEL_BSC && c->have_params, "no BSC parameters on the device");
  REQUIRE(W && pi && sigma, "NULL output");
  if (c->h_theta_fresh) {  // evoamd_mstep_device already brought Theta over
    memcpy(W, c->h_theta + MAILBOX_HDR, (size_t)c->D * c->H * sizeof(double));
    *pi = c->h_dpar[DP_PI];
    *sigma = c->h_dpar[DP_SIGMA];
    return 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_par, c->W, (size_t)c->D * c->H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_dpar, c->dpar, DP_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(W, c->h_par, (size_t)c->D * c->H * sizeof(double));
  *pi = c->h_dpar[DP_PI];
  *sigma = c->h_dpar[DP_SIGMA];
  return 0;
}

extern "C" int evoamd_get_params_sssc(evoamd_ctx *c, double *W, double *pies, double *mus, double *Psi, double *sigma2) {
  REQUIRE(c && c->configured && c->model == EVOAMD_MODEL_SSSC && c->have_params, "no SSSC parameters on the device");
  REQUIRE(W && pies && mus && Psi && sigma2, "NULL output");
  if (c->h_theta_fresh) {  // evoamd_mstep_device already brought Theta over
    const size_t DH = (size_t)c->D * c->H, HH = (size_t)c->H * c->H, H = c->H;
    const double *th = c->h_theta + MAILBOX_HDR;
    memcpy(W, th, DH * sizeof(double));
    memcpy(Psi, th + DH, HH * sizeof(double));
    memcpy(mus, th + DH + HH, H * sizeof(double));
    memcpy(pies, th + DH + HH + H, H * sizeof(double));
    *sigma2 = c->h_dpar[DP_SIGMA2];
    return 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t DH = (size_t)c->D * c->H, HH = (size_t)c->H * c->H, H = c->H;
  double *hw = c->h_par, *hpsi = hw + DH, *hmu = hpsi + HH, *hpi = hmu + 2 * H;
  HIP_TRY(hipMemcpyAsync(hw, c->W, DH * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hpsi, c->Psi, HH * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hmu, c->mus, H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hpi, c->pies, H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_dpar, c->dpar, DP_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(W, hw, DH * sizeof(double));
  memcpy(Psi, hpsi, HH * sizeof(double));
  memcpy(mus, hmu, H * sizeof(double));
  memcpy(pies, hpi, H * sizeof(double));
  *sigma2 = c->h_dpar[DP_SIGMA2];
  return 0;
}

extern "C" int evoamd_free_energy(evoamd_ctx *c, const double *lpj, int64_t N, int C, double *Fs_out) {
  REQUIRE(c && lpj && Fs_out && N > 0 && C > 0, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<double> d;
  TRY(d.alloc((size_t)N * C + 1));
  hipError_t e = hipMemcpyAsync(d, lpj, (size_t)N * C * sizeof(double), hipMemcpyHostToDevice, c->stream);
  int r = 0;
  if (e != hipSuccess) r = fail(EVOAMD_E_HIP, "free_energy upload: %s", hipGetErrorString(e));
  if (!r) r = row_lse(c, d, N, C, nullptr, nullptr, d + (size_t)N * C);
  if (!r) {
    e = hipMemcpyAsync(Fs_out, d + (size_t)N * C, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) r = fail(EVOAMD_E_HIP, "free_energy copy back: %s", hipGetErrorString(e));
  }
  return r;
}

// ---------------------------------------------------------------------------------------
// exact log-likelihood over all 2^Hv states (kernels_exact.hpp): own scratch + the shared-batch scratch, no EM state touched
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_loglik_exact(evoamd_ctx *c, int background, int chunk_states, double *ll_out, double *marg_out,
                                   double *Fs_out) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "configure, upload_data and set_params first");
  REQUIRE(Fs_out, "evoamd_loglik_exact: Fs_out is NULL");
  REQUIRE(background == 0 || background == 1, "evoamd_loglik_exact: background must be 0 or 1");
  const int H = c->H, Hv = H - background;
  if (Hv < 1 || Hv > EXACT_MAX_HV)
    return fail(EVOAMD_E_INVALID, "evoamd_loglik_exact: %d latents vary (H = %d, background = %d); 1 .. %d can be enumerated",
                Hv, H, background, EXACT_MAX_HV);
  const i64 N = c->N;
  const u64 total = 1ull << Hv;  // indices 0 .. 2^Hv - 1 (without background, index 0 is the permanent all-zero state)
  i64 C = chunk_states;
  if (chunk_states != 0) {
    REQUIRE(chunk_states >= 64 && (chunk_states & (chunk_states - 1)) == 0,
            "evoamd_loglik_exact: chunk_states must be 0 (automatic) or a power of two >= 64");
    REQUIRE(N * C < 2147483647LL, "evoamd_loglik_exact: N * chunk_states must fit in int32");
  } else {
    C = 65536;
    while (C > 64 && (N * C * (i64)sizeof(double) > (512ll << 20) || N * C >= 2147483647LL)) C >>= 1;
    REQUIRE(N * C < 2147483647LL, "evoamd_loglik_exact: N * 64 must fit in int32");
    while (C > 64 && (u64)(C >> 1) >= total) C >>= 1;  // no larger than the index space needs
  }
  int logC = 0;
  while ((1ll << logC) < C) logC++;
  const int cmax = (u64)C < total ? (int)C : (int)total;  // states of the largest chunk (Hv < 6: one partial chunk)
  HIP_TRY(hipSetDevice(c->device));
  TRY(c->tmp_states.ensure(c, (size_t)cmax * c->HW));
  TRY(c->tmp_lpj.ensure(c, (size_t)N * cmax));
  TRY(ensure_B(c));
  if (c->model == EVOAMD_MODEL_SSSC) TRY(ensure_lists(c, N * cmax));
  // m (N) | z (N) | ll (N) | Fs (1) | partial (ceil(N / 4)) | a (N x Hv) | marg (N x H)
  const unsigned nb = cdiv(N, 4);
  const size_t need = (size_t)3 * N + 1 + nb + (size_t)N * Hv + (size_t)N * H;
  TRY(c->exact_buf.ensure(c, need));
  double *run_m = c->exact_buf, *run_z = run_m + N, *d_ll = run_z + N, *d_Fs = d_ll + N, *d_part = d_Fs + 1;
  double *run_a = marg_out ? d_part + nb : nullptr, *d_marg = marg_out ? d_part + nb + (size_t)N * Hv : nullptr;
  unsigned *flags = c->flags + c->N;  // the clamp flag words evoamd_lpj_shared borrows
  {
    SpanGuard g(c, KID_MISC);
    if (!background)
      allzero_lpj_kernel<<<cdiv(N, 256), 256, 0, c->stream>>>(c->yy, N, c->dpar, c->model == EVOAMD_MODEL_SSSC, run_m, 1,
                                                              flags, c->err);
    exact_seed_kernel<<<cdiv(N, 256), 256, 0, c->stream>>>(run_m, run_z, run_a, N, Hv, background);
    HIP_TRY(hipGetLastError());
  }
  const LevelHints lv = batch_hints(c, 2);
  for (u64 g0 = 0; g0 < total; g0 += (u64)C) {
    const int cnt = total - g0 < (u64)C ? (int)(total - g0) : (int)C;
    {
      SpanGuard g(c, KID_MISC);
      exact_enumerate_kernel<<<cdiv(cnt, 256), 256, 0, c->stream>>>(c->tmp_states, g0, cnt, Hv, c->HW, background);
      HIP_TRY(hipGetLastError());
    }
    Batch b = {c->tmp_states, nullptr, c->Y, c->Bm, c->yy, N, cnt, 1, c->tmp_lpj, cnt, 0, flags, KID_MISC, 2};
    b.mask = c->mask_infr;
    TRY(launch_lpj(c, b, lv));
    SpanGuard g(c, KID_MISC);
    if (marg_out)
      exact_fold_kernel<true><<<nb, 256, 0, c->stream>>>(c->tmp_lpj, cnt, N, g0, cnt, logC, Hv, !background, run_m, run_z, run_a);
    else
      exact_fold_kernel<false><<<nb, 256, 0, c->stream>>>(c->tmp_lpj, cnt, N, g0, cnt, logC, Hv, !background, run_m, run_z, run_a);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "exact log-likelihood chunk");
  }
  {
    SpanGuard g(c, KID_MISC);
    exact_finish_kernel<<<nb, 256, 0, c->stream>>>(run_m, run_z, run_a, N, Hv, H, d_ll, d_marg, d_part);
    reduce_partials_kernel<<<1, 256, 0, c->stream>>>(d_part, nb, d_Fs, 0);
    HIP_TRY(hipGetLastError());
  }
  if (ll_out) HIP_TRY(hipMemcpyAsync(ll_out, d_ll, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (marg_out) HIP_TRY(hipMemcpyAsync(marg_out, d_marg, (size_t)N * H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(Fs_out, d_Fs, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);  // synchronises the stream
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// overlapping image patches (kernels_patches.hpp): own scratch, no EM state touched
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_patches_extract(evoamd_ctx *c, const double *img, int H, int W, int C, int ph, int pw, int shift,
                                      double *Y_out) {
  REQUIRE(c && img && Y_out, "evoamd_patches_extract: NULL argument");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_extract: %s", msg);
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C, y_n = (size_t)g.N * g.D;
  TRY(c->patch_img.ensure(c, img_n));
  TRY(c->patch_Y.ensure(c, y_n));
  HIP_TRY(hipMemcpyAsync(c->patch_img, img, img_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  {
    SpanGuard sg(c, KID_PATCHES);
    const i64 blocks = (i64)((y_n + 255) / 256);
    patches_extract_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, c->stream>>>(c->patch_img, g, c->patch_Y);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(Y_out, c->patch_Y, y_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// The merge kernels over the estimates `src` serves (PatchRows: dense device rows; PatchSelect: the resident selected
// reconstruction; PatchDrawRows: the resident posterior draws, one per grid row) into `out` on the device: n_img images of
// img_n doubles, image i from grid row i.  Enqueues only.
template <class Src>
static void enqueue_patches_merge(evoamd_ctx *c, const Src &src, const PatchGeom &g, int method, double *out, unsigned n_img) {
  const size_t img_n = (size_t)g.H * g.W * g.C;
  SpanGuard sg(c, KID_PATCHES);
  if (method == 0) {
    patches_mean_kernel<<<dim3(cdiv((i64)img_n, 256), n_img), 256, 0, c->stream>>>(src, g, out);
  } else {
    const int K = patch_max_cover(g);  // <= ph * pw <= 1024
    int P = 1;
    while (P < K) P <<= 1;
    if (P <= 64) {
      const i64 waves = ((i64)img_n + 64 / P - 1) / (64 / P);
      patches_median_kernel<1><<<dim3(cdiv(waves, 4), n_img), 256, 0, c->stream>>>(src, g, P, out);
    } else {
      const dim3 blocks(cdiv((i64)img_n, 4), n_img);  // one wave per output element
      switch (P) {
        case 128: patches_median_kernel<2><<<blocks, 256, 0, c->stream>>>(src, g, P, out); break;
        case 256: patches_median_kernel<4><<<blocks, 256, 0, c->stream>>>(src, g, P, out); break;
        case 512: patches_median_kernel<8><<<blocks, 256, 0, c->stream>>>(src, g, P, out); break;
        default: patches_median_kernel<16><<<blocks, 256, 0, c->stream>>>(src, g, P, out); break;
      }
    }
  }
}

// One image into c->patch_img (which holds img_n doubles), then to the host.
template <class Src>
static int launch_patches_merge(evoamd_ctx *c, const Src &src, const PatchGeom &g, int method, double *img_out) {
  const size_t img_n = (size_t)g.H * g.W * g.C;
  enqueue_patches_merge(c, src, g, method, c->patch_img.get(), 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(img_out, c->patch_img, img_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_patches_merge(evoamd_ctx *c, const double *Y, int H, int W, int C, int ph, int pw, int shift,
                                    int method, double *img_out) {
  REQUIRE(c && Y && img_out, "evoamd_patches_merge: NULL argument");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge: %s", msg);
  REQUIRE(method == 0 || method == 1, "evoamd_patches_merge: method must be 0 (mean) or 1 (median)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C, y_n = (size_t)g.N * g.D;
  TRY(c->patch_img.ensure(c, img_n));
  TRY(c->patch_Y.ensure(c, y_n));
  HIP_TRY(hipMemcpyAsync(c->patch_Y, Y, y_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return launch_patches_merge(c, PatchRows{c->patch_Y}, g, method, img_out);
}

extern "C" int evoamd_patches_merge_weighted(evoamd_ctx *c, const double *Y, const double *V, int H, int W, int C, int ph, int pw,
                                             int shift, double *img_out) {
  REQUIRE(c && Y && V && img_out, "evoamd_patches_merge_weighted: NULL argument");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_weighted: %s", msg);
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C, y_n = (size_t)g.N * g.D;
  TRY(c->patch_img.ensure(c, img_n));
  TRY(c->patch_Y.ensure(c, y_n));
  TRY(c->patch_V.ensure(c, y_n));
  HIP_TRY(hipMemcpyAsync(c->patch_Y, Y, y_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->patch_V, V, y_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  {
    SpanGuard sg(c, KID_PATCHES);
    patches_wmean_kernel<<<cdiv((i64)img_n, 256), 256, 0, c->stream>>>(PatchRows{c->patch_Y}, PatchRows{c->patch_V}, g, c->patch_img);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(img_out, c->patch_img, img_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the selected reconstruction, resident (evoamd_reconstruct_resident / evoamd_patches_merge_resident) ----
static const char *const REC_OUTDATED =
    "no current resident reconstruction: call evoamd_reconstruct_resident after the statistics pass (a later statistics "
    "pass, new parameters, or an upload of data, masks or y_reconstructed outdate it)";

extern "C" int evoamd_reconstruct_resident(evoamd_ctx *c, const uint8_t *x) {
  REQUIRE(c && c->configured && c->have_data && c->have_params, "evoamd_reconstruct_resident: configure, upload data and set parameters first");
  REQUIRE(!c->f32, "reconstruction is not available in the float32 mode");
  HIP_TRY(hipSetDevice(c->device));
  drop_resident_rec(c);
  bool uses_keep = false;
  if (!c->yhat_valid) {
    REQUIRE(c->stats_rows_valid, "evoamd_reconstruct_resident: call evoamd_stats first (and before setting new parameters)");
    TRY(compute_reconstruction(c));
  }
  if (c->mask_infr) {  // incomplete data: the masks are resident, x is not read
    if (!c->yrec_from_pass) {  // the pass ran without reconstruct_in_stats (its M-step read an older y_reconstructed)
      select_rec_kernel<<<cdiv(c->N, 4), 256, 0, c->stream>>>(c->Y, c->ldY, c->mask_x, c->mask_infr, c->yhat, c->N, c->D, c->Yrec,
                                                          c->model == EVOAMD_MODEL_BSC);
      HIP_TRY(hipGetLastError());
      made_yrec_from_pass(c, /*in_stats=*/false);
    }
  } else if (x == EVOAMD_KEEP_RESIDENT) {
    REQUIRE(c->keep_x_valid, "evoamd_reconstruct_resident: EVOAMD_KEEP_RESIDENT, but no keep-mask was uploaded for this geometry");
    uses_keep = true;
  } else if (x) {
    const size_t nd = (size_t)c->N * c->D;
    if (!c->keep_x) TRY(c->keep_x.alloc(nd));
    on_keep_mask(c, /*uploaded=*/false);
    HIP_TRY(hipMemcpyAsync(c->keep_x, x, nd, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // x is pageable host memory of the caller
    on_keep_mask(c, /*uploaded=*/true);
    uses_keep = true;
  }
  made_resident_rec(c, uses_keep);
  return 0;
}

// what the merge gathers from; valid while c->rec_resident
static PatchSelect resident_select(const evoamd_ctx *c) {
  PatchSelect s;
  s.rec = c->mask_infr ? c->Yrec : c->yhat;
  s.Y = c->Y;
  s.ldY = c->ldY;
  s.x = c->mask_infr ? c->mask_x : (c->rec_uses_keep ? c->keep_x : nullptr);
  s.infr = c->mask_infr;
  s.any = c->row_any;
  return s;
}

extern "C" int evoamd_download_reconstruction(evoamd_ctx *c, double *y_hat) {
  REQUIRE(c && y_hat, "evoamd_download_reconstruction: NULL argument");
  if (!(c->configured && c->rec_resident && c->yhat_valid)) return fail(EVOAMD_E_INVALID, "evoamd_download_reconstruction: %s", REC_OUTDATED);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(y_hat, c->yhat, (size_t)c->N * c->D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_patches_merge_resident(evoamd_ctx *c, int H, int W, int C, int ph, int pw, int shift, int method,
                                             double *img_out) {
  REQUIRE(c && img_out, "evoamd_patches_merge_resident: NULL argument");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_resident: %s", msg);
  REQUIRE(method == 0 || method == 1, "evoamd_patches_merge_resident: method must be 0 (mean) or 1 (median)");
  if (!(c->configured && c->rec_resident)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_resident: %s", REC_OUTDATED);
  if (g.N != c->N || g.D != c->D)
    return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_resident: the patch geometry is (N, D) = (%lld, %d), the context holds (%lld, %d)",
                (long long)g.N, g.D, (long long)c->N, c->D);
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C, y_n = (size_t)g.N * g.D;
  const PatchSelect sel = resident_select(c);
  if (c->merge_select_fused) {
    TRY(c->patch_img.ensure(c, img_n));
    return launch_patches_merge(c, sel, g, method, img_out);
  }
  TRY(c->patch_img.ensure(c, img_n));
  TRY(c->patch_Y.ensure(c, y_n));  // select-then-merge (default): y_rec as dense rows, then the kernels of evoamd_patches_merge
  {
    SpanGuard sg(c, KID_PATCHES);
    const i64 blocks = (i64)((y_n + 255) / 256);
    patches_select_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, c->stream>>>(sel, g.N, g.D, c->patch_Y);
  }
  HIP_TRY(hipGetLastError());
  return launch_patches_merge(c, PatchRows{c->patch_Y}, g, method, img_out);
}

// ---- merges of what evoamd_posterior_sample / evoamd_predictive_moments left on the device ----
// Nothing of the EM state or its validity flags is touched; the images go through the patch scratch.
extern "C" int evoamd_patches_merge_samples(evoamd_ctx *c, int H, int W, int C, int ph, int pw, int shift, int method, int t0,
                                            int n_draws, double *imgs_out, double *mean_out, double *std_out) {
  REQUIRE(c, "evoamd_patches_merge_samples: ctx is NULL");
  REQUIRE(imgs_out || mean_out || std_out, "evoamd_patches_merge_samples: imgs_out, mean_out and std_out are all NULL");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_samples: %s", msg);
  REQUIRE(method == 0 || method == 1, "evoamd_patches_merge_samples: method must be 0 (mean) or 1 (median)");
  REQUIRE(c->configured && c->ps_keep >= 0 && c->ps_N == c->N && c->ps_D == c->D,
          "evoamd_patches_merge_samples: no draws on the device (call evoamd_posterior_sample first; a failed call and "
          "evoamd_configure leave none)");
  REQUIRE(c->ps_keep & PSAMP_KEEP_Y, "evoamd_patches_merge_samples: the last evoamd_posterior_sample did not keep y");
  if (g.N != c->ps_N || g.D != c->ps_D)
    return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_samples: the patch geometry is (N, D) = (%lld, %d), the draws are (%lld, %d)",
                (long long)g.N, g.D, (long long)c->ps_N, c->ps_D);
  if (t0 < 0 || n_draws < 1 || (i64)t0 + n_draws > c->ps_T)
    return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_samples: draws %d .. %lld asked for, the last call made T = %lld",
                t0, (long long)t0 + n_draws - 1, (long long)c->ps_T);
  REQUIRE(n_draws <= 65535, "evoamd_patches_merge_samples: at most 65535 draws per call");
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C;
  const bool moments = mean_out || std_out;
  // scratch: [the n images, where they are stored | mean | std]; the mean merger forms the moments without storing images
  const bool store = imgs_out || method == 1;
  const size_t n_store = store ? (size_t)n_draws * img_n : 0;
  TRY(c->patch_img.ensure(c, n_store + 2 * img_n));
  double *imgs = store ? c->patch_img.get() : nullptr;
  double *d_mean = c->patch_img.get() + n_store, *d_std = d_mean + img_n;
  if (method == 0) {
    SpanGuard sg(c, KID_PATCHES);
    patches_mean_draws_kernel<<<cdiv((i64)img_n, 256), 256, 0, c->stream>>>(c->ps_y, c->ps_T, t0, n_draws, g, imgs,
                                                                            mean_out ? d_mean : nullptr, std_out ? d_std : nullptr);
  } else {
    enqueue_patches_merge(c, PatchDrawRows{c->ps_y, c->ps_T, t0}, g, 1, imgs, (unsigned)n_draws);
    if (moments) {
      SpanGuard sg(c, KID_PATCHES);
      patches_moments_kernel<<<cdiv((i64)img_n, 256), 256, 0, c->stream>>>(imgs, n_draws, (i64)img_n, mean_out ? d_mean : nullptr,
                                                                           std_out ? d_std : nullptr);
    }
  }
  HIP_TRY(hipGetLastError());
  if (imgs_out) HIP_TRY(hipMemcpyAsync(imgs_out, imgs, n_store * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (mean_out) HIP_TRY(hipMemcpyAsync(mean_out, d_mean, img_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (std_out) HIP_TRY(hipMemcpyAsync(std_out, d_std, img_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_patches_merge_predictive(evoamd_ctx *c, int H, int W, int C, int ph, int pw, int shift, int what,
                                               double *img_out) {
  REQUIRE(c && img_out, "evoamd_patches_merge_predictive: NULL argument");
  PatchGeom g;
  if (const char *msg = patch_geom_make(H, W, C, ph, pw, shift, &g)) return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_predictive: %s", msg);
  REQUIRE(what >= 0 && what <= 3, "evoamd_patches_merge_predictive: what must be 0 (mean of mean), 1 (median of mean), 2 (precision) or 3 (mean of var)");
  REQUIRE(c->configured && c->pred_N > 0 && c->pred_N == c->N && c->pred_D == c->D,
          "evoamd_patches_merge_predictive: no moments on the device (call evoamd_predictive_moments first; a failed call and "
          "evoamd_configure leave none)");
  if (g.N != c->pred_N || g.D != c->pred_D)
    return fail(EVOAMD_E_INVALID, "evoamd_patches_merge_predictive: the patch geometry is (N, D) = (%lld, %d), the moments are (%lld, %d)",
                (long long)g.N, g.D, (long long)c->pred_N, c->pred_D);
  HIP_TRY(hipSetDevice(c->device));
  const size_t img_n = (size_t)H * W * C, nd = (size_t)c->pred_N * c->pred_D;
  TRY(c->patch_img.ensure(c, img_n));
  const PatchRows mean{c->pred_buf.get()}, var{c->pred_buf.get() + nd};
  if (what != 2) return launch_patches_merge(c, what == 3 ? var : mean, g, what == 1 ? 1 : 0, img_out);
  {
    SpanGuard sg(c, KID_PATCHES);
    patches_wmean_kernel<<<cdiv((i64)img_n, 256), 256, 0, c->stream>>>(mean, var, g, c->patch_img);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(img_out, c->patch_img, img_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// Read-out calls: they read (K^n, lpj, Theta, data) and write only to buffers of their own -- the posterior codes, the
// predictive moments and scores, the posterior samples, the log-likelihood estimate and, further down, the neighbourhood
// bound and the two AIS calls.  What they share stands here once: one admission (readout_admit), one way to hand outputs
// back (fetch_if, download_view) and, for the three calls whose kernels take PredArgs, one builder of the fields that come
// from the context, one R x model dispatch and one tally of the status vector.  Outputs sized by what the caller asks for
// are listed in a FitList.  A call supplies its own refusals, buffers and views, its kernels' own arguments, the validity
// of its results (made_*) and the point at which it drops its earlier ones.
// ---------------------------------------------------------------------------------------
// who: the caller's name in the texts; need_kn: the call reads K^n itself (the codes refuse through kn_gen instead)
static int readout_admit(const evoamd_ctx *c, const char *who, bool need_kn = true) {
  if (!(c && c->configured && c->have_data && c->have_params))
    return fail(EVOAMD_E_INVALID, "%s: configure, upload data and set parameters first", who);
  if (c->f32) return fail(EVOAMD_E_INVALID, "%s is not available in the float32 mode", who);
  if (need_kn) REQUIRE_KN(c);
  return 0;
}

// the optional array of a call: copied where the caller gave a buffer
static hipError_t fetch_if(evoamd_ctx *c, void *dst, const void *src, size_t bytes) {
  return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// the tail of the evoamd_download_* calls: one array a call left on the device, to the host
static int download_view(evoamd_ctx *c, void *out, const void *src, size_t bytes) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the calls on PredArgs (kernels_predictive.hpp): one lane holds R of the D observables
static int pred_admit_D(const evoamd_ctx *c, const char *who) {
  if (c->D > 64 * PRED_R_MAX)
    return fail(EVOAMD_E_INVALID, "%s: D = %d, at most %d observables are supported (64 lanes x %d registers)", who, c->D,
                64 * PRED_R_MAX, PRED_R_MAX);
  return 0;
}

// the PredArgs fields that come straight from the context; the callers set status, add_noise and their outputs, and
// sigma2 through pred_sigma once the scalars are on the host
struct PredLaunch {
  int R = 1;       // observables per lane: the kernels' first template argument
  size_t lds = 0;  // dynamic LDS of a workgroup
};
static PredLaunch fill_pred_args(const evoamd_ctx *c, PredArgs &a) {
  a.mask = c->mask_infr, a.row_any = c->mask_infr ? c->row_any.get() : nullptr;
  a.lpj = c->lpj, a.states = c->states;
  a.Wt = c->pred_Wt, a.G = c->G, a.Psi = c->Psi, a.mus = c->mus, a.Bm = c->Bm;
  a.N = c->N;
  a.D = c->D, a.H = c->H, a.HW = c->HW, a.S = c->S, a.S_perm = c->S_perm, a.L = c->L;
  a.kcap = c->H < PRED_MAX_K ? c->H : PRED_MAX_K;
  a.bg = c->bg_unit;
  PredLaunch l;
  while (64 * l.R < c->D) l.R <<= 1;
  l.lds = PRED_WAVES * pred_lds_doubles(a.kcap, c->model == EVOAMD_MODEL_SSSC) * sizeof(double);
  return l;
}

// dpar: the scalars of the current Theta, fetched by the caller (a device update leaves them in the scalar block only).
// Sets sigma2 and returns sigma.
static double pred_sigma(const evoamd_ctx *c, const double *dpar, PredArgs &a) {
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  a.sigma2 = sssc ? dpar[DP_SIGMA2] : dpar[DP_SIGMA] * dpar[DP_SIGMA];
  return sssc ? sqrt(dpar[DP_SIGMA2]) : dpar[DP_SIGMA];
}

// W^T into pred_Wt; launched inside the caller's SpanGuard, so it counts in the caller's timing class
static void pred_transpose_W(evoamd_ctx *c) {
  transpose_kernel<<<cdiv((i64)c->H * c->D, 256), 256, 0, c->stream>>>(c->W, c->D, c->H, c->pred_Wt);
}

// (R, model) as compile-time constants: launch(r, s) with decltype(r)::value in {1, 2, 4, 8} and decltype(s)::value = ES3C
template <typename Launch>
static void pred_dispatch(int R, bool sssc, Launch launch) {
  auto with_model = [&](auto s) {
    switch (R) {
      case 1: launch(std::integral_constant<int, 1>{}, s); break;
      case 2: launch(std::integral_constant<int, 2>{}, s); break;
      case 4: launch(std::integral_constant<int, 4>{}, s); break;
      default: launch(std::integral_constant<int, 8>{}, s); break;
    }
  };
  if (sssc)
    with_model(std::true_type{});
  else
    with_model(std::false_type{});
}

// The status vector of such a kernel, on the host: the refusal of a state beyond PRED_MAX_K, else counts[0] = singular,
// counts[1] = skipped, counts[2 + i] = the datapoints whose status is extra[i].  counts is written in place.
static int pred_tally(const char *who, const int *status, i64 N, int64_t *counts, std::initializer_list<int> extra = {}) {
  for (size_t k = 0; k < 2 + extra.size(); k++) counts[k] = 0;
  for (i64 n = 0; n < N; n++) {
    const int st = status[(size_t)n];
    if ((st & 0xFF) == PRED_OVER_K)
      return fail(EVOAMD_E_INVALID, "%s: datapoint n = %lld holds a state with k = %d active latents, "
                  "at most %d are supported (PRED_MAX_K)", who, (long long)n, st >> 8, PRED_MAX_K);
    counts[0] += st == PRED_SINGULAR;
    counts[1] += st == PRED_SKIPPED;
    int64_t *cnt = counts + 2;
    for (int code : extra) *cnt++ += st == code;
  }
  return 0;
}

// ---- posterior code readout (kernels_codes.hpp) ----
static const char *const CODES_NEED_STATS = ": call evoamd_stats first (and before setting new parameters or changing K^n)";

static int codes_preamble(evoamd_ctx *c, const char *who) {
  TRY(readout_admit(c, who, /*need_kn=*/false));
  if (!(c->stats_rows_valid && c->rows_kn_gen == c->kn_gen)) return fail(EVOAMD_E_INVALID, "%s%s", who, CODES_NEED_STATS);
  HIP_TRY(hipSetDevice(c->device));
  return 0;
}

extern "C" int evoamd_posterior_codes(evoamd_ctx *c, int max_active, double p_min, int32_t *idx, double *p, double *m,
                                      int32_t *nnz, int32_t *map_slot, double *map_q, uint8_t *map_state_packed) {
  TRY(codes_preamble(c, "evoamd_posterior_codes"));
  REQUIRE(max_active >= 1 && max_active <= CODES_MAX_A, "evoamd_posterior_codes: max_active must be in [1, 64]");
  REQUIRE(p_min >= 0.0, "evoamd_posterior_codes: p_min must be >= 0 (and not NaN)");
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  REQUIRE(sssc || !m, "evoamd_posterior_codes: EBSC has no E_q[s z] (m must be NULL)");
  const size_t N = (size_t)c->N, A = (size_t)max_active, PB = (size_t)(c->H + 7) / 8;
  // p | m | map_q | idx | nnz | map_slot | map_state: descending alignment
  const size_t o_p = 0, o_m = o_p + N * A * 8, o_q = o_m + N * A * 8, o_idx = o_q + N * 8, o_nnz = o_idx + N * A * 4,
               o_slot = o_nnz + N * 4, o_state = o_slot + N * 4, need = o_state + N * PB;
  TRY(c->codes_buf.ensure(c, need));
  uint8_t *b = c->codes_buf;
  CodesArgs a = {};
  a.Es = sssc ? c->Y + c->D : c->Es;
  a.Ez = sssc ? c->Y + c->D + c->H : nullptr;
  a.ldE = sssc ? c->ldY : c->H;
  a.lpj = c->lpj;
  a.states = c->states;
  a.N = c->N;
  a.H = c->H, a.HW = c->HW, a.S = c->S, a.S_perm = c->S_perm, a.L = c->L, a.PB = (int)PB;
  a.A = max_active;
  a.p_min = p_min;
  a.idx = idx ? (int *)(b + o_idx) : nullptr;
  a.p = p ? (double *)(b + o_p) : nullptr;
  a.m = m ? (double *)(b + o_m) : nullptr;
  a.nnz = nnz ? (int *)(b + o_nnz) : nullptr;
  a.map_slot = map_slot ? (int *)(b + o_slot) : nullptr;
  a.map_q = map_q ? (double *)(b + o_q) : nullptr;
  a.map_state = map_state_packed ? b + o_state : nullptr;
  a.err = c->err;
  int home = c->codes_path >= 0 ? c->codes_path : (c->H <= 64 * CODES_R ? CODES_REG : c->H <= CODES_LDS_H ? CODES_LDS : CODES_GMEM);
  REQUIRE(home != CODES_REG || c->H <= 64 * CODES_R, "evoamd_posterior_codes: codes_path 0 (registers) needs H <= 512");
  REQUIRE(home != CODES_LDS || c->H <= CODES_LDS_H, "evoamd_posterior_codes: codes_path 1 (LDS) needs H <= 4096");
  {
    SpanGuard g(c, KID_MISC);
    const unsigned grid = cdiv(c->N, CODES_WAVES);
    if (home == CODES_REG)
      posterior_codes_kernel<CODES_REG><<<grid, 64 * CODES_WAVES, 0, c->stream>>>(a);
    else if (home == CODES_LDS)
      posterior_codes_kernel<CODES_LDS><<<grid, 64 * CODES_WAVES, (size_t)CODES_WAVES * c->H * sizeof(double), c->stream>>>(a);
    else
      posterior_codes_kernel<CODES_GMEM><<<grid, 64 * CODES_WAVES, 0, c->stream>>>(a);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(fetch_if(c, idx, a.idx, N * A * 4));
  HIP_TRY(fetch_if(c, p, a.p, N * A * 8));
  HIP_TRY(fetch_if(c, m, a.m, N * A * 8));
  HIP_TRY(fetch_if(c, nnz, a.nnz, N * 4));
  HIP_TRY(fetch_if(c, map_slot, a.map_slot, N * 4));
  HIP_TRY(fetch_if(c, map_q, a.map_q, N * 8));
  HIP_TRY(fetch_if(c, map_state_packed, a.map_state, N * PB));
  return check_err(c);  // synchronises the stream
}

// The dense rows the codes are cut from: Es (N x H) and, ES3C, Ez (N x H) of the last statistics pass.
extern "C" int evoamd_download_posterior(evoamd_ctx *c, double *Es, double *Ez) {
  TRY(codes_preamble(c, "evoamd_download_posterior"));
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  REQUIRE(sssc || !Ez, "evoamd_download_posterior: EBSC has no E_q[s z] (Ez must be NULL)");
  const size_t w = (size_t)c->H * sizeof(double);
  if (!sssc) {
    if (Es) HIP_TRY(hipMemcpyAsync(Es, c->Es, (size_t)c->N * w, hipMemcpyDeviceToHost, c->stream));
  } else {
    const size_t pitch = (size_t)c->ldY * sizeof(double);
    if (Es) HIP_TRY(hipMemcpy2DAsync(Es, w, c->Y + c->D, pitch, w, (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    if (Ez) HIP_TRY(hipMemcpy2DAsync(Ez, w, c->Y + c->D + c->H, pitch, w, (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// predictive moments (kernels_predictive.hpp): own buffers; of the EM state only B = Y W is (re)formed, like every lpj pass
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_predictive_moments(evoamd_ctx *c, int add_noise, int64_t counters[2]) {
  TRY(readout_admit(c, "evoamd_predictive_moments"));
  REQUIRE(counters, "evoamd_predictive_moments: counters is NULL");
  TRY(pred_admit_D(c, "evoamd_predictive_moments"));
  HIP_TRY(hipSetDevice(c->device));
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  const i64 N = c->N;
  const int D = c->D, H = c->H;
  made_predictive(c, 0);
  if (sssc) TRY(ensure_B(c));
  const size_t nd = (size_t)N * D;
  TRY(c->pred_buf.ensure(c, 2 * nd));
  TRY(c->pred_Wt.ensure(c, (size_t)H * D));
  TRY(c->pred_status.ensure(c, (size_t)N));
  double dpar[DP_COUNT];
  HIP_TRY(hipMemcpyAsync(dpar, c->dpar, DP_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  PredArgs a = {};
  const PredLaunch l = fill_pred_args(c, a);
  pred_sigma(c, dpar, a);
  a.add_noise = add_noise ? 1 : 0;
  a.mean = c->pred_buf;
  a.var = c->pred_buf + nd;
  a.status = c->pred_status;
  {
    SpanGuard g(c, KID_MISC);
    pred_transpose_W(c);
    pred_dispatch(l.R, sssc, [&](auto r, auto s) {
      predictive_kernel<decltype(r)::value, decltype(s)::value><<<cdiv(N, PRED_WAVES), 64 * PRED_WAVES, l.lds, c->stream>>>(a);
    });
  }
  HIP_TRY(hipGetLastError());
  std::vector<int> status((size_t)N);
  HIP_TRY(hipMemcpyAsync(status.data(), c->pred_status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  TRY(pred_tally("evoamd_predictive_moments", status.data(), N, counters));
  made_predictive(c, N);
  c->pred_D = D;
  return 0;
}

extern "C" int evoamd_download_predictive(evoamd_ctx *c, double *mean, double *var) {
  REQUIRE(c, "evoamd_download_predictive: ctx is NULL");
  REQUIRE(c->configured && c->pred_N > 0 && c->pred_N == c->N && c->pred_D == c->D,
          "evoamd_download_predictive: no results on the device (call evoamd_predictive_moments first; a failed call and "
          "evoamd_configure drop them)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t nd = (size_t)c->pred_N * c->pred_D;
  if (mean) HIP_TRY(hipMemcpyAsync(mean, c->pred_buf, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (var) HIP_TRY(hipMemcpyAsync(var, c->pred_buf + nd, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------
// log predictive density and PIT per entry (kernels_predictive_score.hpp has the law): the admission, the Theta scalars,
// the PredArgs and the launch shape of evoamd_predictive_moments; own buffers, sized before anything is launched; the
// moments evoamd_predictive_moments left on the device stay as they are
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_predictive_score(evoamd_ctx *c, const double *y_true, const uint8_t *query, int add_noise,
                                       const evoamd_pred_score_out *out, int64_t counters[4], double total[2]) {
  TRY(readout_admit(c, "evoamd_predictive_score"));
  REQUIRE(y_true && query && counters && total, "evoamd_predictive_score: y_true, query, counters or total is NULL");
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  REQUIRE(sssc || add_noise, "evoamd_predictive_score: EBSC without the noise term has variance 0 at every entry: nothing to score");
  TRY(pred_admit_D(c, "evoamd_predictive_score"));
  HIP_TRY(hipSetDevice(c->device));
  const evoamd_pred_score_out o = out ? *out : evoamd_pred_score_out{};
  REQUIRE(!o.logp == !o.pit, "evoamd_predictive_score: logp and pit come together (both or neither)");
  const i64 N = c->N;
  const int D = c->D, H = c->H;
  const size_t nd = (size_t)N * D, n = (size_t)N;
  const bool per_entry = o.logp != nullptr;
  const unsigned grid = cdiv(N, PRED_WAVES);
  // ---- every buffer, before anything is launched
  TRY(c->pscore_y.ensure(c, nd));
  TRY(c->pscore_q.ensure(c, nd));
  TRY(c->pscore_d.ensure(c, (per_entry ? 2 * nd : 0) + n + 2 * (size_t)grid + 2));
  TRY(c->pscore_i.ensure(c, 3 * n));
  TRY(c->pscore_list.ensure(c, n + 1));
  TRY(c->pred_Wt.ensure(c, (size_t)H * D));
  if (sssc) TRY(ensure_B(c));
  double dpar[DP_COUNT];  // one synchronise for the scalars and the two uploads
  HIP_TRY(hipMemcpyAsync(dpar, c->dpar, DP_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->pscore_y, y_true, nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->pscore_q, query, nd, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  PredScoreArgs q = {};
  PredArgs &a = q.p;
  const PredLaunch l = fill_pred_args(c, a);
  pred_sigma(c, dpar, a);
  a.add_noise = add_noise ? 1 : 0;
  q.y_true = c->pscore_y;
  q.query = c->pscore_q;
  double *dd = c->pscore_d;
  if (per_entry) q.logp = dd, q.pit = dd + nd, dd += 2 * nd;
  q.logp_n = dd;
  double *partial = dd + n, *d_total = partial + 2 * (size_t)grid;
  q.count = c->pscore_i, q.nbad = q.count + n, a.status = q.count + 2 * n;
  q.list = c->pscore_list;
  {
    SpanGuard g(c, KID_PRED_SCORE);
    pred_transpose_W(c);
    pred_score_visit_kernel<<<grid, 64 * PRED_WAVES, 0, c->stream>>>(q);
    pred_score_compact_kernel<<<1, PRED_COMPACT_THREADS, 0, c->stream>>>(a.status, N, q.list);
    pred_dispatch(l.R, sssc, [&](auto r, auto s) {
      predictive_score_kernel<decltype(r)::value, decltype(s)::value><<<grid, 64 * PRED_WAVES, l.lds, c->stream>>>(q);
    });
    pred_score_partials_kernel<<<cdiv((i64)grid, 256), 256, 0, c->stream>>>(q.logp_n, q.count, N, (i64)grid, partial);
    reduce_partials_kernel<<<1, 256, 0, c->stream>>>(partial, (i64)grid, d_total, 0);
    reduce_partials_kernel<<<1, 256, 0, c->stream>>>(partial + grid, (i64)grid, d_total + 1, 0);
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "predictive_score");
  std::vector<int> ints(3 * n);
  HIP_TRY(hipMemcpyAsync(ints.data(), c->pscore_i, 3 * n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int *status = ints.data() + 2 * n, *nbad = ints.data() + n;
  int64_t cnt[4] = {0, 0, 0, 0};  // the caller's counters are written once everything has arrived
  TRY(pred_tally("evoamd_predictive_score", status, N, cnt, {PRED_NOT_QUERIED}));
  for (size_t i = 0; i < n; i++) cnt[3] += nbad[i];
  if (per_entry) {
    HIP_TRY(hipMemcpyAsync(o.logp, q.logp, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(o.pit, q.pit, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(fetch_if(c, o.logp_n, q.logp_n, n * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(total, d_total, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (o.count) memcpy(o.count, ints.data(), n * sizeof(int));
  for (int k = 0; k < 4; k++) counters[k] = cnt[k];
  return 0;
}

// ---------------------------------------------------------------------------------------
// Proposals for K^n: seeding (kernels_seed.hpp, kernels_seed_beam.hpp), local search (kernels_sweep.hpp,
// kernels_sweep_swap.hpp) and the neighbourhood bound that sums what the flip sweep ranks (kernels_nbound.hpp).
// One table of the family's kernels, indexed like their LDS layouts; one admission for what all
// of them refuse; one launch plan (how many wavefronts of a workgroup fit the LDS limit, how large the grid is); one rule
// for the home of the rows of G(n) on masked ES3C; one builder of the SeedArgs fields that come from the context.
// Every refusal comes before the first write.
// ---------------------------------------------------------------------------------------
#define KN_LDS_MAX (150 * 1024)  // dynamic LDS a workgroup of these kernels may ask for
static const void *const kn_kernels[SEED_LDS_KINDS][2] = {  // [SeedLdsKind][ES3C]
    {(const void *)seed_states_kernel<false>, (const void *)seed_states_kernel<true>},
    {(const void *)seed_states_masked_kernel<false>, (const void *)seed_states_masked_kernel<true>},
    {(const void *)seed_states_beam_kernel<false>, (const void *)seed_states_beam_kernel<true>},
    {(const void *)sweep_neighbours_kernel<false>, (const void *)sweep_neighbours_kernel<true>},
    {(const void *)sweep_neighbours_kernel<false, true>, (const void *)sweep_neighbours_kernel<true, true>},
    {(const void *)sweep_swap_kernel<false>, (const void *)sweep_swap_kernel<true>},
    {(const void *)nbound_kernel<false>, (const void *)nbound_kernel<true>},
    {(const void *)nbound_kernel<false, true>, (const void *)nbound_kernel<true, true>}};

static int kn_set_lds_limits() {
  for (const auto &pair : kn_kernels)
    for (const void *f : pair) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, KN_LDS_MAX));
  return 0;
}

// What seeding and sweeping refuse alike, in this order.  who: the caller's name in the texts; masks_refusal: the caller's
// text for resident masks, nullptr when it admits them; need_kn: the call reads K^n.
static int kn_admit(const evoamd_ctx *c, const char *who, const char *masks_refusal, bool need_kn) {
  if (!c->have_params) return fail(EVOAMD_E_INVALID, "%s: no Theta installed (set parameters first)", who);
  if (!c->have_data) return fail(EVOAMD_E_INVALID, "%s: no data (upload data first)", who);
  if (need_kn) REQUIRE_KN(c);
  REQUIRE(!c->mask_infr || !masks_refusal, masks_refusal);
  if (c->bg_unit) return fail(EVOAMD_E_INVALID, "%s: option background_unit is not supported", who);
  if (c->f32) return fail(EVOAMD_E_INVALID, "%s is not available in the float32 mode (ebsc_f32)", who);
  if (c->model != EVOAMD_MODEL_SSSC && c->bsc_direct)
    return fail(EVOAMD_E_INVALID, "%s: bsc_direct keeps no G = W^T W, which the scores need", who);
  return 0;
}

// From one wavefront's share of LDS to the wavefronts of a workgroup and the grid.  W starts at 4 and shrinks until W shares
// fit: by halving everywhere but in the masked flip sweep, which steps down by one.  The difference is inherited and
// unmeasured; it stays, because either rule changed would change a launch shape.
enum KnStep { KN_STEP_HALVE, KN_STEP_DECREMENT };
struct KnLaunch {
  int W = 4;
  size_t wave_bytes = 0;
  unsigned grid = 1;
};
// refusal: the text when one share does not fit; cu_mult: workgroups per CU the grid is capped at
static int kn_plan_launch(const evoamd_ctx *c, size_t wave_bytes, const char *refusal, int cu_mult, KnStep step, KnLaunch &l) {
  REQUIRE(wave_bytes <= KN_LDS_MAX, refusal);
  l.wave_bytes = wave_bytes;
  l.W = 4;
  while (l.W > 1 && l.W * wave_bytes > KN_LDS_MAX) l.W = step == KN_STEP_HALVE ? l.W >> 1 : l.W - 1;
  l.grid = (unsigned)std::min<i64>(cdiv(c->N, l.W), (i64)c->n_cu * cu_mult);
  return 0;
}

// Masked ES3C: the R rows of G(n) a wavefront keeps.  Their home is LDS while one wavefront's share with them fits, else a
// buffer of the context (seed_rows) with fewer workgroups, each wavefront of the grid owning R Hp doubles.
struct KnRows {
  int R = 0, lds = 0;  // lds: the rows whose home is LDS (R or 0)
  int cu_mult = 64;
  size_t doubles(const KnLaunch &l, int Hp) const { return R && !lds ? (size_t)l.grid * l.W * R * Hp : 0; }
};
static KnRows kn_plan_rows(SeedLdsKind kind, SeedLdsShape shape, int R) {
  KnRows r;
  shape.rows_lds = r.R = R;
  r.lds = R && seed_lds_bytes(kind, shape) <= KN_LDS_MAX ? R : 0;
  r.cu_mult = R && !r.lds ? 4 : 64;
  return r;
}

// the SeedArgs fields that come straight from the context; the callers set A / Q / path / lpj_path and rows / R.  Every
// kernel of the family is handed dig, W, mask and D, also those that never read them: the sweeps read no dig, and W, mask
// and D are read by the masked instantiations alone.
static void fill_seed_args(const evoamd_ctx *c, SeedArgs &a) {
  a = SeedArgs{};
  a.states = c->states, a.dig = c->dig;
  a.Bm = c->Bm, a.yy = c->yy;
  a.G = c->G, a.Gd = c->diag;
  a.GP = c->GP, a.GPt = c->seed_gpt;
  a.mus = c->mus, a.pil_bar = c->pilbar_v;
  a.dpar = c->dpar, a.err = c->err;
  a.N = c->N;
  a.S = c->S, a.H = c->H, a.HW = c->HW, a.Hp = (int)cdiv(c->H, 64) * 64;
  a.W = c->W, a.mask = c->mask_infr, a.D = c->D;
}

// which kernel kinds take which argument struct: another pairing is refused, not launched
static bool kn_takes(SeedLdsKind k, const SeedArgs &) { return k == SEED_LDS_GREEDY || k == SEED_LDS_GREEDY_MASKED; }
static bool kn_takes(SeedLdsKind k, const SeedBeamArgs &) { return k == SEED_LDS_BEAM; }
static bool kn_takes(SeedLdsKind k, const SweepArgs &) { return k == SEED_LDS_FLIP || k == SEED_LDS_FLIP_MASKED; }
static bool kn_takes(SeedLdsKind k, const SweepSwapArgs &) { return k == SEED_LDS_SWAP; }
static bool kn_takes(SeedLdsKind k, const NboundArgs &) { return k == SEED_LDS_NBOUND || k == SEED_LDS_NBOUND_MASKED; }
template <class Args>
static int kn_launch(evoamd_ctx *c, SeedLdsKind kind, const KnLaunch &l, const Args &args) {
  REQUIRE(kn_takes(kind, args), "kn_launch: these are not the arguments of this kind of kernel");
  void *argv[] = {const_cast<Args *>(&args)};
  HIP_TRY(hipLaunchKernel(kn_kernels[kind][c->model == EVOAMD_MODEL_SSSC], dim3(l.grid), dim3(64 * l.W), argv,
                          l.W * l.wave_bytes, c->stream));
  return 0;
}

static int kn_transpose_gp(evoamd_ctx *c) {
  seed_transpose_gp_kernel<<<cdiv((i64)c->H * c->H, 256), 256, 0, c->stream>>>(c->GP, c->H, c->seed_gpt);
  return 0;
}

// ---- seeding: greedy forward selection on the model's lpj, or a beam of partial states (beam > 0; complete data only).
// EVOAMD_SEED_INCOMPLETE is a permission: with masks resident the masked kernel runs (the datapoint's own Gram rows from W
// and the mask), without masks the complete kernel, whatever the flag says.
// seed_admit: what the greedy call and the beam call refuse alike, with one text each; masks_refusal as in kn_admit.
static int seed_admit(evoamd_ctx *c, int max_active, const char *masks_refusal) {
  TRY(kn_admit(c, "evoamd_seed_states", masks_refusal, /*need_kn=*/false));
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  const int S = c->S, H = c->H, A = max_active;
  const int cap = sssc ? SEED_MAX_A_SSSC : SEED_MAX_A_BSC;
  if (A < 1 || A > S || A > H || A > cap)
    return fail(EVOAMD_E_INVALID, "evoamd_seed_states: max_active = %d must be in [1, min(S = %d, H = %d, %d)] (%s)", A, S, H,
                cap, sssc ? "ES3C: at most 8" : "EBSC: at most 64");
  const int q_lo = S / A, q_rem = S % A;
  for (int t = 1; t <= A; t++) {
    const int q = q_lo + (t <= q_rem ? 1 : 0);
    if (q > H - (t - 1))
      return fail(EVOAMD_E_INVALID, "evoamd_seed_states: the quota q_%d = %d exceeds the H - (t - 1) = %d latents left at step %d "
                  "(S = %d, max_active = %d)", t, q, H - (t - 1), t, S, A);
  }
  return 0;
}

// the body of evoamd_seed_states_ex (beam = 0) and evoamd_seed_states_beam (beam = B, after its range check)
static int seed_states_run(evoamd_ctx *c, int max_active, int beam, int32_t *path_out, double *lpj_out) {
  const bool sssc = c->model == EVOAMD_MODEL_SSSC, masked = c->mask_infr != nullptr;
  const int S = c->S, H = c->H, A = max_active;
  const int Hp = (int)cdiv(H, 64) * 64, Q = S / A + (S % A ? 1 : 0);
  const SeedLdsKind kind = beam ? SEED_LDS_BEAM : (masked ? SEED_LDS_GREEDY_MASKED : SEED_LDS_GREEDY);
  SeedLdsShape shape = {sssc, Hp, c->HW, Q, A, beam, masked ? c->D : 0, 0, 0};
  // ES3C, masked: the winners' rows of G(n) and its diagonal
  const KnRows rows = kn_plan_rows(kind, shape, masked && sssc ? A : 0);
  shape.rows_lds = rows.lds;
  const size_t wave_bytes = seed_lds_bytes(kind, shape);
  if (beam && wave_bytes > KN_LDS_MAX)
    return fail(EVOAMD_E_INVALID, "evoamd_seed_states_beam: the keys of one datapoint and the two beams (H = %d, beam = %d: %zu "
                "bytes) do not fit one wavefront's share of LDS", H, beam, wave_bytes);
  KnLaunch l;
  TRY(kn_plan_launch(c, wave_bytes,
                     masked ? "evoamd_seed_states: the scores of one datapoint (16 H bytes) and the column of W (12 D "
                              "bytes) do not fit one wavefront's share of LDS"
                            : "evoamd_seed_states: the scores of one datapoint (16 H bytes) do not fit one wavefront's share of LDS",
                     rows.cu_mult, KN_STEP_HALVE, l));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure_B(c));
  const size_t n_out = (size_t)c->N * A;
  const size_t out_bytes = ((n_out * sizeof(int) + 7) / 8) * 8;
  if (path_out || lpj_out) TRY(c->stage.ensure(c, out_bytes + n_out * sizeof(double)));
  if (sssc) TRY(c->seed_gpt.ensure(c, (size_t)H * H));
  if (rows.doubles(l, Hp)) TRY(c->seed_rows.ensure(c, rows.doubles(l, Hp)));
  SeedBeamArgs b;
  SeedArgs &a = b.sd;  // (the greedy kernels take the SeedArgs alone)
  fill_seed_args(c, a);
  a.A = A, a.Q = Q;
  a.path = path_out ? (int *)c->stage.get() : nullptr;
  a.lpj_path = lpj_out ? (double *)(c->stage.get() + out_bytes) : nullptr;
  a.rows = rows.doubles(l, Hp) ? c->seed_rows.get() : nullptr;
  a.R = rows.R;
  b.B = beam;
  on_kn_changed(c, KN_BY_CALLER);
  {
    SpanGuard g(c, KID_SEED_STATES);
    if (sssc) TRY(kn_transpose_gp(c));
    TRY(beam ? kn_launch(c, kind, l, b) : kn_launch(c, kind, l, a));
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, beam ? "seed_states_beam" : "seed_states");
  if (path_out) HIP_TRY(hipMemcpyAsync(path_out, a.path, n_out * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (lpj_out) HIP_TRY(hipMemcpyAsync(lpj_out, a.lpj_path, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  on_kn_complete(c);
  return 0;
}

extern "C" int evoamd_seed_states_ex(evoamd_ctx *c, int max_active, unsigned flags, int32_t *path_out, double *lpj_out) {
  REQUIRE(c && c->configured, "configure first");
  // (a missing Theta or missing data is named before an unknown flag)
  REQUIRE(!(flags & ~(unsigned)EVOAMD_SEED_INCOMPLETE) || !c->have_params || !c->have_data, "evoamd_seed_states_ex: unknown flag");
  TRY(seed_admit(c, max_active, (flags & EVOAMD_SEED_INCOMPLETE) ? nullptr : "evoamd_seed_states: incomplete data (masks present) "
                 "is not supported (evoamd_seed_states_ex with EVOAMD_SEED_INCOMPLETE)"));
  return seed_states_run(c, max_active, 0, path_out, lpj_out);
}

extern "C" int evoamd_seed_states(evoamd_ctx *c, int max_active, int32_t *path_out, double *lpj_out) {
  return evoamd_seed_states_ex(c, max_active, 0u, path_out, lpj_out);
}

// K^n seeded by a beam of partial states (kernels_seed_beam.hpp has the law).  Complete data only.
extern "C" int evoamd_seed_states_beam(evoamd_ctx *c, int max_active, int beam, int32_t *path_out, double *lpj_out) {
  REQUIRE(c && c->configured, "configure first");
  TRY(seed_admit(c, max_active, "evoamd_seed_states_beam: incomplete data (masks present) is not supported: beam seeding is "
                 "for complete data"));
  if (beam < 1 || beam > c->S / max_active || beam > SEED_BEAM_MAX)
    return fail(EVOAMD_E_INVALID, "evoamd_seed_states_beam: beam = %d must be in [1, min(S / max_active = %d, %d)] (every beam "
                "member is a stored state; SEED_BEAM_MAX = %d)", beam, c->S / max_active, SEED_BEAM_MAX, SEED_BEAM_MAX);
  return seed_states_run(c, max_active, beam, path_out, lpj_out);
}

// ---- local search on K^n: the one-flip and the swap neighbours of its best states (kernels_sweep.hpp and
// kernels_sweep_swap.hpp have the laws).  A sweep is the proposal kernels into the resident candidate batch, the model's own
// lpj of the emitted rows and the selection; the lpj rows of K^n stay what a pass over it would give.
// EVOAMD_SWEEP_INCOMPLETE is a permission, like EVOAMD_SEED_INCOMPLETE: with masks resident the masked instantiation runs (the
// datapoint's own Gram quantities from W and the mask), without masks the complete one, whatever the flag says.
struct SweepPlan {
  KnLaunch flip, swap;  // the flip stage; the swap stage (EVOAMD_SWEEP_SWAP)
  bool masked = false;
  KnRows rows;          // masked ES3C: the SWEEP_ROWS rows of G(n) per wavefront
  unsigned nb = 0;      // the EVOAMD_SWEEP_SWAP / EVOAMD_SWEEP_NO_FLIP bits, 0 = flips only
};

// admits: the flag bits the entry point knows -- 0 (the plain calls), EVOAMD_SWEEP_INCOMPLETE (_ex) or all three (_nb)
static int sweep_plan(const evoamd_ctx *c, int n_parents, int n_keep, unsigned flags, unsigned admits, SweepPlan &p) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(!(flags & ~admits), "sweep: unknown flag");
  REQUIRE((flags & EVOAMD_SWEEP_SWAP) || !(flags & EVOAMD_SWEEP_NO_FLIP),
          "sweep: EVOAMD_SWEEP_NO_FLIP is valid only together with EVOAMD_SWEEP_SWAP");
  REQUIRE(!(flags & EVOAMD_SWEEP_SWAP) || !(flags & EVOAMD_SWEEP_INCOMPLETE),
          "sweep: EVOAMD_SWEEP_SWAP together with EVOAMD_SWEEP_INCOMPLETE: swaps on incomplete data are not supported");
  TRY(kn_admit(c, "sweep", (flags & EVOAMD_SWEEP_INCOMPLETE) ? nullptr : "sweep: incomplete data (masks present) is not supported",
               /*need_kn=*/true));
  if (n_parents < 1 || n_parents > c->S || n_parents > SWEEP_MAX_P)
    return fail(EVOAMD_E_INVALID, "sweep: n_parents = %d must be in [1, min(S = %d, %d)]", n_parents, c->S, SWEEP_MAX_P);
  REQUIRE(n_keep >= 1, "sweep: n_keep must be positive");
  if ((i64)n_parents * n_keep > c->Cmax)
    return fail(EVOAMD_E_INVALID, "sweep: n_parents * n_keep = %lld exceeds the configured Cmax = %d", (long long)n_parents * n_keep,
                c->Cmax);
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  p.masked = c->mask_infr != nullptr;
  const SeedLdsKind kind = p.masked ? SEED_LDS_FLIP_MASKED : SEED_LDS_FLIP;
  SeedLdsShape shape = {sssc, (int)cdiv(c->H, 64) * 64, c->HW, n_keep, 0, 0, p.masked ? c->D : 0, 0, c->S};
  p.rows = kn_plan_rows(kind, shape, p.masked && sssc ? SWEEP_ROWS : 0);
  shape.rows_lds = p.rows.lds;
  TRY(kn_plan_launch(c, seed_lds_bytes(kind, shape),
                     p.masked ? "sweep: the keys of one datapoint (8 or 24 H bytes), the staged column of W (8 D bytes) and the "
                                "list of the reliable entries (4 D bytes) do not fit one wavefront's share of LDS"
                              : "sweep: the keys of one datapoint (8 or 16 H bytes) do not fit one wavefront's share of LDS",
                     p.rows.cu_mult, p.masked ? KN_STEP_DECREMENT : KN_STEP_HALVE, p.flip));
  p.nb = flags & (EVOAMD_SWEEP_SWAP | EVOAMD_SWEEP_NO_FLIP);
  if (!p.nb) return 0;
  // the swap stage: the quota of two stages and the swap kernel's share of LDS
  if (!(flags & EVOAMD_SWEEP_NO_FLIP) && (i64)2 * n_parents * n_keep > c->Cmax)
    return fail(EVOAMD_E_INVALID, "sweep: 2 * n_parents * n_keep = %lld (flips and swaps, n_keep rows per parent each) exceeds the "
                                  "configured Cmax = %d", (long long)2 * n_parents * n_keep, c->Cmax);
  return kn_plan_launch(c, seed_lds_bytes(SEED_LDS_SWAP, shape),
                        "sweep: the keys of one datapoint (8 or 16 H bytes), the running lists of the swap stage "
                        "(32 n_keep bytes) and the held pairs (4 S bytes) do not fit one wavefront's share of LDS",
                        64, KN_STEP_HALVE, p.swap);
}

// the buffers a sweep needs, B = Y W, (ES3C) the transpose of GP: once per call, Theta stays fixed
static int sweep_prepare(evoamd_ctx *c, const SweepPlan &p) {
  const size_t N = (size_t)c->N;
  TRY(ensure_B(c));
  if (p.nb) {
    TRY(c->swap_d.ensure(c, N));
    TRY(c->swap_i.ensure(c, 3 * N));
  }
  const size_t rows = p.rows.doubles(p.flip, (int)cdiv(c->H, 64) * 64);
  if (rows) TRY(c->seed_rows.ensure(c, rows));
  TRY(c->sweep_d.ensure(c, N * c->Cmax + N));
  TRY(c->sweep_i.ensure(c, 2 * N));
  if (c->model == EVOAMD_MODEL_SSSC) {
    TRY(ensure_lists(c, c->N * (i64)c->Cmax));
    TRY(c->seed_gpt.ensure(c, (size_t)c->H * c->H));
    SpanGuard g(c, KID_SWEEP);
    TRY(kn_transpose_gp(c));
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// ---- one sweep's proposals: the kernels, then the lpj of the emitted rows ("nothing known" level hints)
static int sweep_propose_stage(evoamd_ctx *c, const SweepPlan &p, int n_parents, int n_keep, bool want_score) {
  const size_t N = (size_t)c->N;
  SweepSwapArgs b = {};
  SweepArgs &a = b.sw;  // (the flip kernels take the SweepArgs alone)
  fill_seed_args(c, a.sd);
  a.sd.Q = n_keep;
  if (p.masked) {
    a.sd.R = p.rows.R;
    a.sd.rows = p.rows.R && !p.rows.lds ? c->seed_rows.get() : nullptr;
  }
  a.lpj = c->lpj;
  a.cand = c->cand, a.cand_dig = (c->use_digest && c->cand_dig) ? c->cand_dig.get() : nullptr, a.counts = c->cand_counts;
  a.score = want_score ? c->sweep_d.get() : nullptr;
  a.gain = c->sweep_d + N * c->Cmax;
  a.best_flip = c->sweep_i, a.n_capped = c->sweep_i + N;
  a.L = c->L, a.S_perm = c->S_perm, a.P = n_parents, a.q = n_keep, a.Cmax = c->Cmax;
  if (want_score && (p.nb & EVOAMD_SWEEP_NO_FLIP))
    HIP_TRY(hipMemsetAsync(c->sweep_d, 0xFF, N * c->Cmax * sizeof(double), c->stream));  // rows not emitted: NaN
  if (!(p.nb & EVOAMD_SWEEP_NO_FLIP)) {
    SpanGuard g(c, KID_SWEEP);
    if (want_score) HIP_TRY(hipMemsetAsync(c->sweep_d, 0xFF, N * c->Cmax * sizeof(double), c->stream));  // rows not emitted: NaN
    TRY(kn_launch(c, p.masked ? SEED_LDS_FLIP_MASKED : SEED_LDS_FLIP, p.flip, a));
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sweep proposals");
  }
  if (p.nb & EVOAMD_SWEEP_SWAP) {  // the swap stage: its rows go behind the flip stage's
    b.swap_gain = c->swap_d;
    b.best_swap = c->swap_i, b.n_capped_swap = c->swap_i + 2 * N;
    b.append = (p.nb & EVOAMD_SWEEP_NO_FLIP) ? 0 : 1;
    SpanGuard g(c, KID_SWEEP_SWAP);
    TRY(kn_launch(c, SEED_LDS_SWAP, p.swap, b));
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "sweep swap proposals");
  }
  on_cand_installed(c, /*near_parents=*/false);
  TRY(eval_candidates(c));
  made_cand_lpj(c);
  return 0;
}

// the outputs of the stages that ran, each where the caller gave a buffer; score: only evoamd_sweep_propose_* return it
static int sweep_fetch(evoamd_ctx *c, const SweepPlan &p, const evoamd_sweep_out &o, bool score) {
  const size_t N = (size_t)c->N;
  const bool flips = !(p.nb & EVOAMD_SWEEP_NO_FLIP), swaps = (p.nb & EVOAMD_SWEEP_SWAP) != 0;
  if (swaps && o.best_swap) HIP_TRY(hipMemcpyAsync(o.best_swap, c->swap_i, 2 * N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (swaps && o.swap_gain) HIP_TRY(hipMemcpyAsync(o.swap_gain, c->swap_d, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (swaps && o.n_capped_swap)
    HIP_TRY(hipMemcpyAsync(o.n_capped_swap, c->swap_i + 2 * N, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (score && o.score) HIP_TRY(hipMemcpyAsync(o.score, c->sweep_d, N * c->Cmax * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (flips && o.gain) HIP_TRY(hipMemcpyAsync(o.gain, c->sweep_d + N * c->Cmax, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (flips && o.best_flip) HIP_TRY(hipMemcpyAsync(o.best_flip, c->sweep_i, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (flips && o.n_capped) HIP_TRY(hipMemcpyAsync(o.n_capped, c->sweep_i + N, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (c->model == EVOAMD_MODEL_SSSC) return check_err(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// the body of evoamd_sweep_propose / _ex / _nb
static int sweep_propose_run(evoamd_ctx *c, int n_parents, int n_keep, unsigned flags, unsigned admits, const evoamd_sweep_out &o) {
  SweepPlan p;
  TRY(sweep_plan(c, n_parents, n_keep, flags, admits, p));
  HIP_TRY(hipSetDevice(c->device));
  TRY(sweep_prepare(c, p));
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));
  TRY(sweep_propose_stage(c, p, n_parents, n_keep, o.score != nullptr));
  return sweep_fetch(c, p, o, /*score=*/true);
}

// the body of evoamd_sweep_states / _ex / _nb
static int sweep_states_run(evoamd_ctx *c, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet, unsigned flags,
                            unsigned admits, double *trace_out, int *n_done_out, const evoamd_sweep_out &o) {
  SweepPlan p;
  TRY(sweep_plan(c, n_parents, n_keep, flags, admits, p));
  TRY(estep_check_mprime(c, Mprime));
  REQUIRE(n_sweeps >= 1, "evoamd_sweep_states: n_sweeps must be positive");
  REQUIRE(trace_out && n_done_out, "evoamd_sweep_states: trace_out / n_done_out is NULL");
  HIP_TRY(hipSetDevice(c->device));
  TRY(sweep_prepare(c, p));
  TRY(c->refine_trace.ensure(c, (size_t)3 * n_sweeps));
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));  // after it the selection kernel keeps the rows current (evoamd_refine_states)
  TRY(refine_trace(c, -1, REFINE_TRACE_ZERO));
  int done = 0, copied = 0;
  while (done < n_sweeps) {
    TRY(sweep_propose_stage(c, p, n_parents, n_keep, false));
    TRY(estep_select(c, Mprime, nullptr));
    TRY(refine_trace(c, done, REFINE_TRACE_ROW));
    done++;
    if (stop_when_quiet) {  // the row of this sweep: the one wait of the loop
      HIP_TRY(hipMemcpyAsync(trace_out + 3 * copied, c->refine_trace + 3 * copied, 3 * sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      copied = done;
      if (trace_out[3 * (done - 1) + 2] <= 0.0) break;
    }
  }
  TRY(refine_trace(c, done - 1, REFINE_TRACE_RESTORE));
  if (copied < done)
    HIP_TRY(hipMemcpyAsync(trace_out + 3 * copied, c->refine_trace + 3 * copied, (size_t)3 * (done - copied) * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  *n_done_out = done;
  return sweep_fetch(c, p, o, /*score=*/false);
}

// The three generations of the sweep ABI forward to the two bodies: the plain calls admit no flag, the _ex calls
// EVOAMD_SWEEP_INCOMPLETE (the swap bits are unknown flags to them), the _nb calls all three.
static evoamd_sweep_out sweep_flip_out(double *score, int32_t *best_flip, double *gain, int32_t *n_capped) {
  evoamd_sweep_out o = {};
  o.score = score, o.best_flip = best_flip, o.gain = gain, o.n_capped = n_capped;
  return o;
}
static const unsigned SWEEP_NB_FLAGS = EVOAMD_SWEEP_INCOMPLETE | EVOAMD_SWEEP_SWAP | EVOAMD_SWEEP_NO_FLIP;

extern "C" int evoamd_sweep_propose(evoamd_ctx *c, int n_parents, int n_keep, double *score_out, int32_t *best_flip_out,
                                    double *gain_out, int32_t *n_capped_out) {
  return sweep_propose_run(c, n_parents, n_keep, 0u, 0u, sweep_flip_out(score_out, best_flip_out, gain_out, n_capped_out));
}

extern "C" int evoamd_sweep_propose_ex(evoamd_ctx *c, int n_parents, int n_keep, unsigned flags, double *score_out,
                                       int32_t *best_flip_out, double *gain_out, int32_t *n_capped_out) {
  return sweep_propose_run(c, n_parents, n_keep, flags, EVOAMD_SWEEP_INCOMPLETE,
                           sweep_flip_out(score_out, best_flip_out, gain_out, n_capped_out));
}

extern "C" int evoamd_sweep_propose_nb(evoamd_ctx *c, int n_parents, int n_keep, unsigned flags, const evoamd_sweep_out *out) {
  return sweep_propose_run(c, n_parents, n_keep, flags, SWEEP_NB_FLAGS, out ? *out : evoamd_sweep_out{});
}

extern "C" int evoamd_sweep_states(evoamd_ctx *c, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                                   double *trace_out, int *n_done_out, int32_t *best_flip_out, double *gain_out,
                                   int32_t *n_capped_out) {
  return sweep_states_run(c, n_sweeps, n_parents, n_keep, Mprime, stop_when_quiet, 0u, 0u, trace_out, n_done_out,
                          sweep_flip_out(nullptr, best_flip_out, gain_out, n_capped_out));
}

extern "C" int evoamd_sweep_states_ex(evoamd_ctx *c, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                                      unsigned flags, double *trace_out, int *n_done_out, int32_t *best_flip_out,
                                      double *gain_out, int32_t *n_capped_out) {
  return sweep_states_run(c, n_sweeps, n_parents, n_keep, Mprime, stop_when_quiet, flags, EVOAMD_SWEEP_INCOMPLETE, trace_out,
                          n_done_out, sweep_flip_out(nullptr, best_flip_out, gain_out, n_capped_out));
}

extern "C" int evoamd_sweep_states_nb(evoamd_ctx *c, int n_sweeps, int n_parents, int n_keep, int Mprime, int stop_when_quiet,
                                      unsigned flags, double *trace_out, int *n_done_out, const evoamd_sweep_out *out) {
  return sweep_states_run(c, n_sweeps, n_parents, n_keep, Mprime, stop_when_quiet, flags, SWEEP_NB_FLAGS, trace_out, n_done_out,
                          out ? *out : evoamd_sweep_out{});
}

// ---- the neighbourhood bound (kernels_nbound.hpp has the law): the one-flip neighbours of the n_parents best states of K^n,
// summed.  A reading of K^n at fixed Theta: the resident rows are evaluated as a sweep does at entry; K^n, the candidate
// batch and the statistics rows are not written.  EVOAMD_NBOUND_INCOMPLETE is a permission, like EVOAMD_SWEEP_INCOMPLETE.
extern "C" int evoamd_neighbour_bound(evoamd_ctx *c, int n_parents, unsigned flags, const evoamd_nbound_out *out) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(!(flags & ~(unsigned)EVOAMD_NBOUND_INCOMPLETE), "evoamd_neighbour_bound: unknown flag");
  TRY(kn_admit(c, "evoamd_neighbour_bound",
               (flags & EVOAMD_NBOUND_INCOMPLETE) ? nullptr : "evoamd_neighbour_bound: incomplete data (masks present) is not "
                                                              "supported without EVOAMD_NBOUND_INCOMPLETE",
               /*need_kn=*/true));
  if (n_parents < 1 || n_parents > c->S)
    return fail(EVOAMD_E_INVALID, "evoamd_neighbour_bound: n_parents = %d must be in [1, S = %d]", n_parents, c->S);
  const bool sssc = c->model == EVOAMD_MODEL_SSSC, masked = c->mask_infr != nullptr;
  const int Hp = (int)cdiv(c->H, 64) * 64;
  const SeedLdsKind kind = masked ? SEED_LDS_NBOUND_MASKED : SEED_LDS_NBOUND;
  SeedLdsShape shape = {sssc, Hp, c->HW, 0, 0, 0, masked ? c->D : 0, 0, c->S};
  const KnRows rows = kn_plan_rows(kind, shape, masked && sssc ? SWEEP_ROWS : 0);
  shape.rows_lds = rows.lds;
  KnLaunch l;
  TRY(kn_plan_launch(c, seed_lds_bytes(kind, shape),
                     masked ? "evoamd_neighbour_bound: the keys of one datapoint (8 or 24 H bytes), the parents and their ranks (8 S "
                              "bytes), the staged column of W (8 D bytes) and the list of the reliable entries (4 D bytes) do not "
                              "fit one wavefront's share of LDS"
                            : "evoamd_neighbour_bound: the keys of one datapoint (8 or 16 H bytes) and the parents and their ranks "
                              "(8 S bytes) do not fit one wavefront's share of LDS",
                     rows.cu_mult, masked ? KN_STEP_DECREMENT : KN_STEP_HALVE, l));
  HIP_TRY(hipSetDevice(c->device));
  const size_t N = (size_t)c->N;
  TRY(ensure_B(c));
  if (rows.doubles(l, Hp)) TRY(c->seed_rows.ensure(c, rows.doubles(l, Hp)));
  TRY(c->nbound_d.ensure(c, 4 * N));
  TRY(c->nbound_i.ensure(c, 4 * N));
  if (sssc) TRY(c->seed_gpt.ensure(c, (size_t)c->H * c->H));
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));
  NboundArgs a = {};
  fill_seed_args(c, a.sd);
  if (masked) {
    a.sd.R = rows.R;
    a.sd.rows = rows.R && !rows.lds ? c->seed_rows.get() : nullptr;
  }
  a.lpj = c->lpj;
  a.F = c->nbound_d, a.M = a.F + N, a.F_plus = a.F + 2 * N, a.best_score = a.F + 3 * N;
  a.n_states = c->nbound_i, a.n_capped = a.n_states + N, a.best_parent = a.n_states + 2 * N, a.best_flip = a.n_states + 3 * N;
  a.L = c->L, a.S_perm = c->S_perm, a.P = n_parents;
  {
    SpanGuard g(c, KID_NBOUND);
    if (sssc) TRY(kn_transpose_gp(c));
    posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                        c->HW, a.F, nullptr, nullptr, nullptr, nullptr);
    TRY(kn_launch(c, kind, l, a));
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "neighbour bound");
  }
  std::vector<double> fp(N);
  HIP_TRY(hipMemcpyAsync(fp.data(), a.F_plus, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  const evoamd_nbound_out o = out ? *out : evoamd_nbound_out{};
  HIP_TRY(fetch_if(c, o.F, a.F, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.M, a.M, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.best_score, a.best_score, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.n_states, a.n_states, N * sizeof(int)));
  HIP_TRY(fetch_if(c, o.n_capped, a.n_capped, N * sizeof(int)));
  HIP_TRY(fetch_if(c, o.best_parent, a.best_parent, N * sizeof(int)));
  HIP_TRY(fetch_if(c, o.best_flip, a.best_flip, N * sizeof(int)));
  if (sssc)
    TRY(check_err(c));  // synchronises the stream
  else
    HIP_TRY(hipStreamSynchronize(c->stream));
  if (o.sum) {  // over the rows with an estimate, in datapoint order
    double sum = 0.0, count = 0.0;
    for (size_t n = 0; n < N; n++)
      if (fp[n] == fp[n]) sum += fp[n], count += 1.0;
    o.sum[0] = sum, o.sum[1] = count;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// annealed importance sampling (kernels_ais.hpp has the law): EBSC; incomplete data under EVOAMD_AIS_INCOMPLETE.  Plan (every refusal, the launch
// shape, the sizes), then the named stages: buffers, chains, fold, (admit) emission + candidate lpj + selection, fetch.
// Without EVOAMD_AIS_ADMIT nothing of the EM state is written: B = Y W is (re)formed like by every lpj pass, nothing else.
// ---------------------------------------------------------------------------------------
// What evoamd_ais_loglik and evoamd_ais_posterior refuse alike, in this order (who: the caller's name in the texts): the
// context and the chain counts in ais_admit, the schedule in ais_check_betas.  Two functions, because evoamd_ais_posterior
// has refusals of its own (n_keep) between them.
// incomplete: the caller's EVOAMD_AIS_INCOMPLETE -- a permission: with masks resident the call takes the masked route
// (*masked), without masks it changes nothing.
static int ais_admit(const evoamd_ctx *c, const char *who, int n_chains, int n_temps, bool incomplete, bool *masked) {
  if (!c->have_params) return fail(EVOAMD_E_INVALID, "%s: no Theta installed (set parameters first)", who);
  if (!c->have_data) return fail(EVOAMD_E_INVALID, "%s: no data (upload data first)", who);
  if (c->model != EVOAMD_MODEL_BSC)
    return fail(EVOAMD_E_INVALID, "%s: ES3C is not supported (a collapsed Gibbs step needs a bordered k x k system per flip); the "
                "call is for EBSC", who);
  if (c->f32)
    return fail(EVOAMD_E_INVALID, "%s is not available in the float32 mode (ebsc_f32): the chains run on the double B = Y W", who);
  if (c->bg_unit) return fail(EVOAMD_E_INVALID, "%s: option background_unit is not supported (every latent is scanned)", who);
  if (c->bsc_direct) return fail(EVOAMD_E_INVALID, "%s: bsc_direct keeps no G = W^T W, whose rows the Gibbs scan reads", who);
  if (c->mask_infr && !incomplete)
    return fail(EVOAMD_E_INVALID, "%s: incomplete data (masks resident) is not supported: the chains need one G for all datapoints", who);
  if (c->H > 64 * AIS_MAX_NC)
    return fail(EVOAMD_E_INVALID, "%s: H = %d, at most %d latents are supported (64 lanes x %d registers of c_j)", who, c->H,
                64 * AIS_MAX_NC, AIS_MAX_NC);
  if (n_chains < 1) return fail(EVOAMD_E_INVALID, "%s: n_chains = %d must be positive", who, n_chains);
  if (n_temps < 1) return fail(EVOAMD_E_INVALID, "%s: n_temps = %d must be positive", who, n_temps);
  *masked = c->mask_infr != nullptr;
  return 0;
}
// the masked route's LDS (per wavefront the rows of Hp doubles, the column and the list over D) against a CU's 160 KiB
#define AIS_LDS_LIMIT (160u << 10)
static int ais_check_masked_lds(const evoamd_ctx *c, const char *who, size_t lds) {
  if (lds > AIS_LDS_LIMIT)
    return fail(EVOAMD_E_INVALID, "%s: incomplete data with D = %d and H = %d needs %zu bytes of LDS per workgroup (per wavefront "
                "the column and the list over D beside the rows over H), above the %u of a compute unit", who, c->D, c->H, lds,
                AIS_LDS_LIMIT);
  return 0;
}
static int ais_check_betas(const char *who, int n_temps, const double *betas) {
  if (!betas) return fail(EVOAMD_E_INVALID, "%s: betas is NULL", who);
  if (betas[0] != 0.0) return fail(EVOAMD_E_INVALID, "%s: betas must start at 0 (betas[0] = %g)", who, betas[0]);
  if (betas[n_temps] != 1.0) return fail(EVOAMD_E_INVALID, "%s: betas must end at 1 (betas[%d] = %g)", who, n_temps, betas[n_temps]);
  for (int t = 1; t <= n_temps; t++)
    if (!(betas[t] >= betas[t - 1]) || (t == 1 && !(betas[1] > 0.0)))
      return fail(EVOAMD_E_INVALID, "%s: betas must not descend and must leave 0 at once (betas[%d] = %g after %g)", who, t, betas[t],
                  betas[t - 1]);
  return 0;
}
// the end of both fetch stages: waits for the stream, the chains' error word with the copies
static int ais_wait(evoamd_ctx *c, const char *who) {
  HIP_TRY(hipMemcpyAsync(c->h_err, c->err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->h_err[0] & EVO_ERR_BAD_ENTRY) {  // guard_index replaced a latent index that was out of range
    HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int), c->stream));
    return fail(EVOAMD_E_INVALID, "internal: %s: a latent index of a chain was out of range", who);
  }
  return 0;
}

struct AisPlan {
  bool reverse = false, admit = false, masked = false;
  size_t lds = 0;  // masked: dynamic LDS of the chain kernel
  int C = 0, T = 0, nc = 1;  // nc: the chunk count the kernel is instantiated for (1, 2, 4, 8, 16)
  unsigned grid = 1;
  size_t n_d = 0, n_i = 0, n_s = 0;  // elements of ais_d / ais_i / ais_s
};

static int ais_plan(const evoamd_ctx *c, int n_chains, int n_temps, const double *betas, unsigned flags, const uint64_t *s_start,
                    int Mprime, AisPlan &p) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(!(flags & ~(unsigned)(EVOAMD_AIS_REVERSE | EVOAMD_AIS_ADMIT | EVOAMD_AIS_INCOMPLETE)), "evoamd_ais_loglik: unknown flag");
  TRY(ais_admit(c, "evoamd_ais_loglik", n_chains, n_temps, (flags & EVOAMD_AIS_INCOMPLETE) != 0, &p.masked));
  TRY(ais_check_betas("evoamd_ais_loglik", n_temps, betas));
  if (p.masked) {
    p.lds = ais_masked_lds_bytes(c->HW, c->D);
    TRY(ais_check_masked_lds(c, "evoamd_ais_loglik", p.lds));
  }
  p.reverse = (flags & EVOAMD_AIS_REVERSE) != 0, p.admit = (flags & EVOAMD_AIS_ADMIT) != 0;
  REQUIRE(!p.reverse || s_start, "evoamd_ais_loglik: EVOAMD_AIS_REVERSE needs s_start, the (N, HW) words of the starting states");
  REQUIRE(!(p.reverse && p.admit), "evoamd_ais_loglik: EVOAMD_AIS_ADMIT with EVOAMD_AIS_REVERSE: a reverse chain ends at the prior, "
                                   "its final states are no proposals for K^n");
  if (p.admit) {
    REQUIRE_KN(c);
    TRY(estep_check_mprime(c, Mprime));
  }
  REQUIRE((i64)c->N * n_chains < 2147483647LL, "evoamd_ais_loglik: N * n_chains must fit in int32");
  p.C = n_chains, p.T = n_temps;
  while (p.nc < c->HW) p.nc <<= 1;
  const size_t N = (size_t)c->N, NC = N * (size_t)n_chains;
  p.grid = (unsigned)std::min<i64>(cdiv((i64)NC, AIS_WAVES), (i64)c->n_cu * 64);
  p.n_d = (size_t)n_temps + 1 + NC + 7 * N;
  p.n_i = NC;
  p.n_s = NC * c->HW + N * c->HW;
  return 0;
}

template <bool REV>
static void ais_launch_chains(evoamd_ctx *c, const AisPlan &p, const AisArgs &a) {
  const size_t lds = (size_t)(1 + AIS_WAVES) * 64 * c->HW * sizeof(double);  // G_jj, then B_n. per wavefront
  switch (p.nc) {
    case 1: ais_chain_kernel<1, REV><<<p.grid, 64 * AIS_WAVES, lds, c->stream>>>(a); break;
    case 2: ais_chain_kernel<2, REV><<<p.grid, 64 * AIS_WAVES, lds, c->stream>>>(a); break;
    case 4: ais_chain_kernel<4, REV><<<p.grid, 64 * AIS_WAVES, lds, c->stream>>>(a); break;
    case 8: ais_chain_kernel<8, REV><<<p.grid, 64 * AIS_WAVES, lds, c->stream>>>(a); break;
    default: ais_chain_kernel<AIS_MAX_NC, REV><<<p.grid, 64 * AIS_WAVES, lds, c->stream>>>(a); break;
  }
}

// incomplete data: the MASKED instantiations; above 64 KiB the dynamic LDS limit is raised once per instantiation
template <int NC, bool REV>
static int ais_launch_masked_one(evoamd_ctx *c, const AisPlan &p, const AisArgs &a, unsigned bit) {
  if (REV) bit <<= 8;
  if (p.lds > (64u << 10) && !(c->ais_lds_set & bit)) {
    HIP_TRY(hipFuncSetAttribute((const void *)ais_chain_kernel<NC, REV, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AIS_LDS_LIMIT));
    c->ais_lds_set |= bit;
  }
  ais_chain_kernel<NC, REV, true><<<p.grid, 64 * AIS_WAVES, p.lds, c->stream>>>(a);
  return 0;
}
template <bool REV>
static int ais_launch_masked(evoamd_ctx *c, const AisPlan &p, const AisArgs &a) {
  switch (p.nc) {
    case 1: return ais_launch_masked_one<1, REV>(c, p, a, 1u);
    case 2: return ais_launch_masked_one<2, REV>(c, p, a, 2u);
    case 4: return ais_launch_masked_one<4, REV>(c, p, a, 4u);
    case 8: return ais_launch_masked_one<8, REV>(c, p, a, 8u);
    default: return ais_launch_masked_one<AIS_MAX_NC, REV>(c, p, a, 16u);
  }
}

// the views into the call's buffers
struct AisBufs {
  double *betas, *log_w, *ll, *ess, *lw_mean, *lw_min, *lw_max, *F_before, *F_after;
  int *flips;
  u64 *fin, *s_start;
  i64 *n_flips;
};
static AisBufs ais_views(const evoamd_ctx *c, const AisPlan &p) {
  const size_t N = (size_t)c->N, NC = N * (size_t)p.C;
  AisBufs b;
  b.betas = c->ais_d, b.log_w = b.betas + p.T + 1, b.ll = b.log_w + NC, b.ess = b.ll + N, b.lw_mean = b.ess + N;
  b.lw_min = b.lw_mean + N, b.lw_max = b.lw_min + N, b.F_before = b.lw_max + N, b.F_after = b.F_before + N;
  b.flips = c->ais_i;
  b.fin = c->ais_s, b.s_start = b.fin + NC * c->HW;
  b.n_flips = c->ais_nf;
  return b;
}

// ---- stage: every buffer, before anything is launched
static int ais_prepare(evoamd_ctx *c, const AisPlan &p) {
  TRY(ensure_B(c));
  TRY(c->ais_d.ensure(c, p.n_d));
  TRY(c->ais_i.ensure(c, p.n_i));
  TRY(c->ais_s.ensure(c, p.n_s));
  TRY(c->ais_nf.ensure(c, (size_t)c->N));
  return 0;
}

// ---- stage: the chains and the fold over them
static int ais_chains_stage(evoamd_ctx *c, const AisPlan &p, const double *betas, uint64_t seed, uint64_t first_index,
                            const uint64_t *s_start) {
  const AisBufs b = ais_views(c, p);
  HIP_TRY(hipMemcpyAsync(b.betas, betas, ((size_t)p.T + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (p.reverse)
    HIP_TRY(hipMemcpyAsync(b.s_start, s_start, (size_t)c->N * c->HW * sizeof(u64), hipMemcpyHostToDevice, c->stream));
  AisArgs a = {};
  a.Bm = c->Bm, a.yy = c->yy, a.G = c->G, a.Gd = c->diag, a.dpar = c->dpar;
  a.betas = b.betas, a.s_start = p.reverse ? b.s_start : nullptr;
  a.log_w = b.log_w, a.fin = b.fin, a.flips = b.flips, a.err = c->err;
  a.N = c->N, a.C = p.C, a.T = p.T, a.H = c->H, a.HW = c->HW;
  a.seed = seed, a.first_index = first_index;
  if (p.masked) a.W = c->W, a.mask = c->mask_infr, a.D = c->D;
  SpanGuard g(c, KID_AIS);
  if (p.masked)
    TRY(p.reverse ? ais_launch_masked<true>(c, p, a) : ais_launch_masked<false>(c, p, a));
  else if (p.reverse)
    ais_launch_chains<true>(c, p, a);
  else
    ais_launch_chains<false>(c, p, a);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "ais chains");
  ais_fold_kernel<<<cdiv(c->N, 256), 256, 0, c->stream>>>(b.log_w, b.flips, c->N, p.C, p.reverse ? 1 : 0, c->H, c->dpar, b.ll, b.ess,
                                                          b.lw_mean, b.lw_min, b.lw_max, b.n_flips);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "ais fold");
  return 0;
}

// ---- stage (admit): the final states as a candidate batch, their lpj from the model's own kernels, the selection --
// the tail of a sweep; F before and after from posterior_score_kernel
static int ais_admit_stage(evoamd_ctx *c, const AisPlan &p, int Mprime, double sums[2]) {
  const AisBufs b = ais_views(c, p);
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));
  posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                      c->HW, b.F_before, nullptr, nullptr, nullptr, nullptr);
  {
    SpanGuard g(c, KID_AIS);
    ais_admit_kernel<<<cdiv(c->N, 256), 256, 0, c->stream>>>(b.fin, c->N, p.C, c->HW, c->Cmax, c->cand,
                                                             (c->use_digest && c->cand_dig) ? c->cand_dig.get() : nullptr, c->cand_counts);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "ais admit");
  }
  on_cand_installed(c, /*near_parents=*/false);
  TRY(eval_candidates(c));
  made_cand_lpj(c);
  TRY(estep_select(c, Mprime, sums));
  posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                      c->HW, b.F_after, nullptr, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- stage: the outputs, each where the caller gave a buffer; sum over the datapoints in their order
static int ais_fetch(evoamd_ctx *c, const AisPlan &p, const evoamd_ais_out &o) {
  const AisBufs b = ais_views(c, p);
  const size_t N = (size_t)c->N, NC = N * (size_t)p.C;
  std::vector<double> ll(N);
  HIP_TRY(hipMemcpyAsync(ll.data(), b.ll, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(fetch_if(c, o.ess, b.ess, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_mean, b.lw_mean, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_min, b.lw_min, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_max, b.lw_max, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.n_flips, b.n_flips, N * sizeof(i64)));
  HIP_TRY(fetch_if(c, o.log_w, b.log_w, NC * sizeof(double)));
  HIP_TRY(fetch_if(c, o.final_words, b.fin, NC * c->HW * sizeof(u64)));
  HIP_TRY(fetch_if(c, o.chain_flips, b.flips, NC * sizeof(int)));
  if (p.admit) HIP_TRY(fetch_if(c, o.F_before, b.F_before, N * sizeof(double)));
  if (p.admit) HIP_TRY(fetch_if(c, o.F_after, b.F_after, N * sizeof(double)));
  TRY(ais_wait(c, "evoamd_ais_loglik"));
  if (o.ll) memcpy(o.ll, ll.data(), N * sizeof(double));
  if (o.sum) {
    double s = 0.0;
    for (size_t n = 0; n < N; n++) s += ll[n];
    o.sum[0] = s;
  }
  return 0;
}

extern "C" int evoamd_ais_loglik(evoamd_ctx *c, int n_chains, int n_temps, const double *betas, uint64_t seed, uint64_t first_index,
                                 unsigned flags, const uint64_t *s_start, int Mprime, const evoamd_ais_out *out) {
  AisPlan p;
  TRY(ais_plan(c, n_chains, n_temps, betas, flags, s_start, Mprime, p));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ais_prepare(c, p));
  TRY(ais_chains_stage(c, p, betas, seed, first_index, s_start));
  const evoamd_ais_out o = out ? *out : evoamd_ais_out{};
  double sums[2] = {0.0, 0.0};
  if (p.admit) {
    TRY(ais_admit_stage(c, p, Mprime, sums));
    if (o.admit_sums) o.admit_sums[0] = sums[0], o.admit_sums[1] = sums[1];
  }
  return ais_fetch(c, p, o);
}

// ---------------------------------------------------------------------------------------
// posterior expectations from the AIS chains (kernels_ais_post.hpp has the law): EBSC; incomplete data under the flag
// EVOAMD_AIS_INCOMPLETE of evoamd_ais_posterior_ex.  Plan (every
// refusal, the launch shape, the block of datapoints, the sizes), then the named stages: buffers, chains + fold block by
// block, the product for `mean`, fetch.  Nothing of the EM state is written, y_hat and its validity included: B = Y W is
// (re)formed like by every lpj pass, nothing else.
// ---------------------------------------------------------------------------------------
// evoamd_ais_posterior_sel: the rows of every per-datapoint output are the n listed datapoints in list order (n = N and
// row = datapoint without a list); with admit the stages emission + candidate lpj + selection + tally follow the fold.
struct AisPostPlan {
  bool masked = false, listed = false, admit = false;
  int C = 0, T = 0, K = 0, nc = 1;  // nc: the chunk count the kernel is instantiated for (1, 2, 4, 8, 16)
  i64 n = 0;                        // rows: listed datapoints, or N
  i64 block = 1;                    // rows per block
  bool mean = false;
  size_t lds = 0;
  size_t n_d = 0, n_rows = 0, n_i = 0, n_s = 0, n_nf = 0;  // elements of aisp_d / aisp_rows / aisp_i / aisp_s / aisp_nf
};

// the list of evoamd_ais_posterior_sel and of the probe: strictly ascending within [0, N); the first offender is named
static int ais_post_check_index(const evoamd_ctx *c, const char *who, const int64_t *index, int64_t n_index) {
  if (n_index < 0) return fail(EVOAMD_E_INVALID, "%s: n_index = %lld must not be negative", who, (long long)n_index);
  if (!index) {
    if (n_index > 0) return fail(EVOAMD_E_INVALID, "%s: index is NULL with n_index = %lld", who, (long long)n_index);
    return 0;
  }
  for (int64_t i = 0; i < n_index; i++) {
    if (index[i] < 0 || index[i] >= c->N)
      return fail(EVOAMD_E_INVALID, "%s: index[%lld] = %lld is outside [0, N = %lld)", who, (long long)i, (long long)index[i], (long long)c->N);
    if (i > 0 && index[i] == index[i - 1])
      return fail(EVOAMD_E_INVALID, "%s: index[%lld] = %lld is repeated (a datapoint is listed once)", who, (long long)i, (long long)index[i]);
    if (i > 0 && index[i] < index[i - 1])
      return fail(EVOAMD_E_INVALID, "%s: index[%lld] = %lld descends (after %lld): the list is ascending", who, (long long)i,
                  (long long)index[i], (long long)index[i - 1]);
  }
  return 0;
}

// sel: the call is evoamd_ais_posterior_sel (index / n_index / Mprime are read, EVOAMD_AIS_ADMIT is a known flag)
static int ais_post_plan(const evoamd_ctx *c, int n_chains, int n_temps, int n_keep, const double *betas, int64_t block_datapoints,
                         unsigned flags, bool mean, AisPostPlan &p, bool sel = false, const int64_t *index = nullptr,
                         int64_t n_index = 0, int Mprime = 1) {
  REQUIRE(c && c->configured, "configure first");
  if (sel)
    REQUIRE(!(flags & ~(unsigned)(EVOAMD_AIS_INCOMPLETE | EVOAMD_AIS_ADMIT)), "evoamd_ais_posterior_sel: unknown flag");
  else
    REQUIRE(!(flags & ~(unsigned)EVOAMD_AIS_INCOMPLETE), "evoamd_ais_posterior_ex: unknown flag");
  TRY(ais_admit(c, "evoamd_ais_posterior", n_chains, n_temps, (flags & EVOAMD_AIS_INCOMPLETE) != 0, &p.masked));
  p.n = c->N;
  if (sel) {
    TRY(ais_post_check_index(c, "evoamd_ais_posterior_sel", index, n_index));
    p.listed = index != nullptr, p.admit = (flags & EVOAMD_AIS_ADMIT) != 0;
    if (p.listed) p.n = n_index;
    if (p.admit) {
      if (c->kn_lost)
        return fail(EVOAMD_E_INVALID, "evoamd_ais_posterior_sel: EVOAMD_AIS_ADMIT needs K^n on the device (evoamd_init_states stopped "
                    "at its round cap: upload or initialise K^n first)");
      if (Mprime < 1 || Mprime > c->S)
        return fail(EVOAMD_E_INVALID, "evoamd_ais_posterior_sel: Mprime = %d must be in [1, S = %d]", Mprime, c->S);
    }
  }
  if (n_keep < 1) return fail(EVOAMD_E_INVALID, "evoamd_ais_posterior: n_keep = %d must be positive", n_keep);
  REQUIRE((i64)n_temps + n_keep < 2147483647LL, "evoamd_ais_posterior: n_temps + n_keep must fit in int32");
  TRY(ais_check_betas("evoamd_ais_posterior", n_temps, betas));
  REQUIRE((i64)c->N * n_chains < 2147483647LL, "evoamd_ais_posterior: N * n_chains must fit in int32");
  const size_t row = (size_t)n_chains * 64 * c->HW;  // doubles of one datapoint's rows
  const i64 fit = (i64)(AIS_POST_ROWS_BYTES / (row * sizeof(double)));
  if (block_datapoints < 0) return fail(EVOAMD_E_INVALID, "evoamd_ais_posterior: block_datapoints = %lld must not be negative", (long long)block_datapoints);
  if (fit < 1 || block_datapoints > fit)
    return fail(EVOAMD_E_INVALID, "evoamd_ais_posterior: the per-chain rows of one block (%lld datapoints x %d chains x %d doubles) exceed %llu MiB",
                (long long)std::max<i64>(block_datapoints, 1), n_chains, 64 * c->HW, (unsigned long long)(AIS_POST_ROWS_BYTES >> 20));
  p.C = n_chains, p.T = n_temps, p.K = n_keep, p.mean = mean;
  while (p.nc < c->HW) p.nc <<= 1;
  p.block = std::max<i64>(std::min<i64>(block_datapoints > 0 ? block_datapoints : fit, p.n), 1);
  p.lds = p.masked ? ais_post_masked_lds_bytes(c->HW, c->D) : ais_post_lds_bytes(c->HW);
  if (p.masked) TRY(ais_check_masked_lds(c, "evoamd_ais_posterior", p.lds));
  const size_t N = (size_t)p.n, NC = N * (size_t)n_chains;
  p.n_d = (size_t)n_temps + 1 + 3 * NC + 2 * N * c->H + 7 * N + (mean ? N * c->D : 0);
  p.n_rows = (size_t)p.block * row;
  p.n_i = NC;
  p.n_s = NC * c->HW + N * c->HW;
  p.n_nf = N + (p.listed ? N : 0);  // n_flips | the list
  if (p.admit) {  // F_before | F_after (n each) | F of every datapoint (N); key (n, C) | five counts and map_held twice (n each)
    p.n_d += 2 * N + (size_t)c->N;
    p.n_i += NC + 6 * N;
  }
  return 0;
}

// the views into the call's buffers (N: the rows of the plan)
struct AisPostBufs {
  double *betas, *log_w, *best_lpj, *wts, *p, *p_se, *count, *map_lpj, *ll, *ess, *lw_mean, *lw_min, *lw_max, *mean;
  double *F_before, *F_after, *F_full;  // admit
  int *flips;
  int *key, *n_distinct, *n_new, *n_proposed, *n_admitted, *held_before, *held_after;  // admit
  u64 *best, *map_state;
  i64 *n_flips, *index;  // index: listed
};
static AisPostBufs ais_post_views(const evoamd_ctx *c, const AisPostPlan &p) {
  const size_t N = (size_t)p.n, NC = N * (size_t)p.C, NH = N * (size_t)c->H;
  AisPostBufs b;
  // (p, p_se and mean first: the product for `mean` reads 16-byte vectors where the operands allow it)
  b.p = c->aisp_d, b.p_se = b.p + NH, b.mean = b.p_se + NH, b.betas = b.mean + (p.mean ? N * (size_t)c->D : 0);
  b.log_w = b.betas + p.T + 1, b.best_lpj = b.log_w + NC, b.wts = b.best_lpj + NC, b.count = b.wts + NC;
  b.map_lpj = b.count + N, b.ll = b.map_lpj + N, b.ess = b.ll + N, b.lw_mean = b.ess + N, b.lw_min = b.lw_mean + N;
  b.lw_max = b.lw_min + N;
  b.F_before = b.lw_max + N, b.F_after = b.F_before + N, b.F_full = b.F_after + N;
  b.flips = c->aisp_i;
  b.key = b.flips + NC, b.n_distinct = b.key + NC, b.n_new = b.n_distinct + N, b.n_proposed = b.n_new + N;
  b.n_admitted = b.n_proposed + N, b.held_before = b.n_admitted + N, b.held_after = b.held_before + N;
  b.best = c->aisp_s, b.map_state = b.best + NC * c->HW;
  b.n_flips = c->aisp_nf, b.index = b.n_flips + N;
  return b;
}

template <int NC>
static int ais_post_launch_one(evoamd_ctx *c, const AisPostPlan &p, const AisPostArgs &a, unsigned grid, unsigned bit) {
  if (p.lds > (64u << 10) && !(c->aisp_lds_set & bit)) {  // once per instantiation
    HIP_TRY(hipFuncSetAttribute((const void *)ais_post_chain_kernel<NC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    c->aisp_lds_set |= bit;
  }
  if constexpr (NC == 1) {  // (its LDS stays far below 64 KiB) without a list: the instantiation that reads no index
    if (!a.index) {
      ais_post_chain_kernel<1, false, true><<<grid, 64 * AIS_WAVES, p.lds, c->stream>>>(a);
      return 0;
    }
  }
  ais_post_chain_kernel<NC><<<grid, 64 * AIS_WAVES, p.lds, c->stream>>>(a);
  return 0;
}
// incomplete data: the MASKED instantiations (their bits of aisp_lds_set: 8 up)
template <int NC>
static int ais_post_launch_masked_one(evoamd_ctx *c, const AisPostPlan &p, const AisPostArgs &a, unsigned grid, unsigned bit) {
  bit <<= 8;
  if (p.lds > (64u << 10) && !(c->aisp_lds_set & bit)) {
    HIP_TRY(hipFuncSetAttribute((const void *)ais_post_chain_kernel<NC, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AIS_LDS_LIMIT));
    c->aisp_lds_set |= bit;
  }
  ais_post_chain_kernel<NC, true><<<grid, 64 * AIS_WAVES, p.lds, c->stream>>>(a);
  return 0;
}
static int ais_post_launch_chains(evoamd_ctx *c, const AisPostPlan &p, const AisPostArgs &a) {
  const unsigned grid = (unsigned)std::min<i64>(cdiv(a.nb * (i64)p.C, AIS_WAVES), (i64)c->n_cu * 64);
  if (p.masked) switch (p.nc) {
      case 1: return ais_post_launch_masked_one<1>(c, p, a, grid, 1u);
      case 2: return ais_post_launch_masked_one<2>(c, p, a, grid, 2u);
      case 4: return ais_post_launch_masked_one<4>(c, p, a, grid, 4u);
      case 8: return ais_post_launch_masked_one<8>(c, p, a, grid, 8u);
      default: return ais_post_launch_masked_one<AIS_MAX_NC>(c, p, a, grid, 16u);
    }
  switch (p.nc) {
    case 1: return ais_post_launch_one<1>(c, p, a, grid, 1u);
    case 2: return ais_post_launch_one<2>(c, p, a, grid, 2u);
    case 4: return ais_post_launch_one<4>(c, p, a, grid, 4u);
    case 8: return ais_post_launch_one<8>(c, p, a, grid, 8u);
    default: return ais_post_launch_one<AIS_MAX_NC>(c, p, a, grid, 16u);
  }
}

// ---- stage: every buffer, before anything is launched
static int ais_post_prepare(evoamd_ctx *c, const AisPostPlan &p) {
  TRY(ensure_B(c));
  TRY(c->aisp_d.ensure(c, p.n_d));
  TRY(c->aisp_rows.ensure(c, p.n_rows));
  TRY(c->aisp_i.ensure(c, p.n_i));
  TRY(c->aisp_s.ensure(c, p.n_s));
  TRY(c->aisp_nf.ensure(c, p.n_nf));
  return 0;
}

// ---- stage: block by block, the chains and the fold over them
// (rb_host: where the caller wants the rows r_c., (N, C, H) on the host -- each block's leave before the next one overwrites them)
// (index: the caller's list when the plan is listed -- the blocks then run over list positions, and the chain kernel reads
// the source datapoint of a row from the list)
static int ais_post_chains_stage(evoamd_ctx *c, const AisPostPlan &p, const double *betas, uint64_t seed, uint64_t first_index,
                                 double *rb_host, const int64_t *index = nullptr) {
  const AisPostBufs b = ais_post_views(c, p);
  HIP_TRY(hipMemcpyAsync(b.betas, betas, ((size_t)p.T + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (p.listed) HIP_TRY(hipMemcpyAsync(b.index, index, (size_t)p.n * sizeof(i64), hipMemcpyHostToDevice, c->stream));
  AisPostArgs a = {};
  a.G = c->G, a.Gd = c->diag, a.dpar = c->dpar, a.betas = b.betas, a.rb = c->aisp_rows, a.err = c->err;
  a.C = p.C, a.T = p.T, a.K = p.K, a.H = c->H, a.HW = c->HW;
  a.seed = seed;
  if (p.masked) a.W = c->W, a.D = c->D;
  AisPostFoldArgs f = {};
  f.log_w = b.log_w, f.best_lpj = b.best_lpj, f.best = b.best, f.flips = b.flips, f.rb = c->aisp_rows, f.dpar = c->dpar;
  f.wts = b.wts, f.p = b.p, f.p_se = b.p_se, f.count = b.count, f.map_lpj = b.map_lpj, f.ll = b.ll, f.ess = b.ess;
  f.lw_mean = b.lw_mean, f.lw_min = b.lw_min, f.lw_max = b.lw_max, f.map_state = b.map_state, f.n_flips = b.n_flips;
  f.C = p.C, f.H = c->H, f.HW = c->HW;
  SpanGuard g(c, KID_AIS_POST);
  for (i64 n0 = 0; n0 < p.n; n0 += p.block) {
    a.nb = f.nb = std::min<i64>(p.block, p.n - n0);
    f.n0 = n0;
    const size_t i0 = (size_t)n0 * p.C;  // the chain kernel sees its block alone
    if (p.listed) {  // ... of the list: the data are those of the whole shard
      a.index = b.index + n0, a.Bm = c->Bm, a.yy = c->yy, a.first_index = first_index;
      if (p.masked) a.mask = c->mask_infr;
    } else {
      a.Bm = c->Bm + (size_t)n0 * c->H, a.yy = c->yy + n0, a.first_index = first_index + (uint64_t)n0;
      if (p.masked) a.mask = c->mask_infr + (size_t)n0 * c->D;
    }
    a.log_w = b.log_w + i0, a.best_lpj = b.best_lpj + i0, a.best = b.best + i0 * c->HW, a.flips = b.flips + i0;
    TRY(ais_post_launch_chains(c, p, a));
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "ais_post chains");
    ais_post_fold_kernel<<<cdiv(a.nb, AIS_WAVES), 64 * AIS_WAVES, 0, c->stream>>>(f);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "ais_post fold");
    if (rb_host)
      HIP_TRY(hipMemcpy2DAsync(rb_host + (size_t)n0 * p.C * c->H, (size_t)c->H * sizeof(double), c->aisp_rows.get(),
                               (size_t)64 * c->HW * sizeof(double), (size_t)c->H * sizeof(double), (size_t)a.nb * p.C,
                               hipMemcpyDeviceToHost, c->stream));
  }
  return 0;
}

// ---- stage: mean = p W^T, the route of compute_reconstruction, into the call's own buffer (never c->yhat)
static int ais_post_mean_stage(evoamd_ctx *c, const AisPostPlan &p) {
  const AisPostBufs b = ais_post_views(c, p);
  SpanGuard g(c, KID_GEMM);
  // (listed: the kernel the call over all N datapoints takes, so that a row has that call's bits)
  launch_gemm_nn_raw(c, b.p, c->H, c->Wt, c->D, b.mean, c->D, p.n, c->D, c->H, nullptr, 0, p.listed ? c->N : 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- stage: the outputs, each where the caller gave a buffer
static int ais_post_fetch(evoamd_ctx *c, const AisPostPlan &p, const evoamd_ais_post_out &o) {
  const AisPostBufs b = ais_post_views(c, p);
  const size_t N = (size_t)p.n, NC = N * (size_t)p.C, H = (size_t)c->H;
  HIP_TRY(fetch_if(c, o.p, b.p, N * H * sizeof(double)));
  HIP_TRY(fetch_if(c, o.p_se, b.p_se, N * H * sizeof(double)));
  HIP_TRY(fetch_if(c, o.count, b.count, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.map_lpj, b.map_lpj, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.map_state, b.map_state, N * c->HW * sizeof(u64)));
  HIP_TRY(fetch_if(c, o.ll, b.ll, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.ess, b.ess, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_mean, b.lw_mean, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_min, b.lw_min, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w_max, b.lw_max, N * sizeof(double)));
  HIP_TRY(fetch_if(c, o.n_flips, b.n_flips, N * sizeof(i64)));
  if (p.mean) HIP_TRY(fetch_if(c, o.mean, b.mean, N * c->D * sizeof(double)));
  HIP_TRY(fetch_if(c, o.log_w, b.log_w, NC * sizeof(double)));
  HIP_TRY(fetch_if(c, o.chain_map_lpj, b.best_lpj, NC * sizeof(double)));
  HIP_TRY(fetch_if(c, o.chain_map_state, b.best, NC * c->HW * sizeof(u64)));
  HIP_TRY(fetch_if(c, o.chain_flips, b.flips, NC * sizeof(int)));
  return ais_wait(c, "evoamd_ais_posterior");
}

extern "C" int evoamd_ais_posterior(evoamd_ctx *c, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                                    uint64_t first_index, int64_t block_datapoints, const evoamd_ais_post_out *out) {
  return evoamd_ais_posterior_ex(c, n_chains, n_temps, n_keep, betas, seed, first_index, block_datapoints, 0u, out);
}

extern "C" int evoamd_ais_posterior_ex(evoamd_ctx *c, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                                       uint64_t first_index, int64_t block_datapoints, unsigned flags,
                                       const evoamd_ais_post_out *out) {
  const evoamd_ais_post_out o = out ? *out : evoamd_ais_post_out{};
  AisPostPlan p;
  TRY(ais_post_plan(c, n_chains, n_temps, n_keep, betas, block_datapoints, flags, o.mean != nullptr, p));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ais_post_prepare(c, p));
  TRY(ais_post_chains_stage(c, p, betas, seed, first_index, o.rb));
  if (p.mean) TRY(ais_post_mean_stage(c, p));
  return ais_post_fetch(c, p, o);
}

// the arguments of the emission and of the tally, from the call's buffers (F_out / map_held: the caller names the side)
static AisPostAdmitArgs ais_post_admit_args(const evoamd_ctx *c, const AisPostPlan &p, const AisPostBufs &b) {
  AisPostAdmitArgs a = {};
  a.best_lpj = b.best_lpj, a.best = b.best, a.index = p.listed ? b.index : nullptr, a.states = c->states;
  a.cand = c->cand, a.cand_dig = (c->use_digest && c->cand_dig) ? c->cand_dig.get() : nullptr, a.cand_counts = c->cand_counts;
  a.key = b.key, a.n_distinct = b.n_distinct, a.n_new = b.n_new, a.n_proposed = b.n_proposed, a.n_admitted = b.n_admitted;
  a.n = p.n, a.C = p.C, a.S = c->S, a.HW = c->HW, a.Cmax = c->Cmax;
  return a;
}

// the emission alone: cand_counts cleared (0 outside the list), then one wavefront per row
static int ais_post_emit(evoamd_ctx *c, const AisPostAdmitArgs &a) {
  SpanGuard g(c, KID_AIS_POST);
  HIP_TRY(hipMemsetAsync(c->cand_counts, 0, (size_t)c->N * sizeof(int), c->stream));
  if (a.n > 0) ais_post_admit_kernel<<<cdiv(a.n, AIS_POST_ADMIT_WAVES), 64 * AIS_POST_ADMIT_WAVES, 0, c->stream>>>(a);
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "ais_post admit");
  return 0;
}

// ---- stage (admit): the resident rows and F before, the emission, the tail of a sweep (candidate lpj, selection), F after
// and the tally
static int ais_post_admit_stage(evoamd_ctx *c, const AisPostPlan &p, int Mprime, double sums[2]) {
  const AisPostBufs b = ais_post_views(c, p);
  on_estep_route(c, /*fused=*/false);
  TRY(estep_resident_pass(c));
  posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                      c->HW, b.F_full, nullptr, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  AisPostAdmitArgs a = ais_post_admit_args(c, p, b);
  a.F_full = b.F_full, a.F_out = b.F_before, a.map_held = b.held_before;
  TRY(ais_post_emit(c, a));
  on_cand_installed(c, /*near_parents=*/false);
  TRY(eval_candidates(c));
  made_cand_lpj(c);
  TRY(estep_select(c, Mprime, sums));
  posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                      c->HW, b.F_full, nullptr, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  a.F_out = b.F_after, a.map_held = b.held_after;
  {
    SpanGuard g(c, KID_AIS_POST);
    ais_post_tally_kernel<<<cdiv(p.n, AIS_POST_ADMIT_WAVES), 64 * AIS_POST_ADMIT_WAVES, 0, c->stream>>>(a);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "ais_post tally");
  }
  return 0;
}

extern "C" int evoamd_ais_posterior_sel(evoamd_ctx *c, int n_chains, int n_temps, int n_keep, const double *betas, uint64_t seed,
                                        uint64_t first_index, int64_t block_datapoints, unsigned flags, const int64_t *index,
                                        int64_t n_index, int Mprime, const evoamd_ais_post_sel_out *out) {
  const evoamd_ais_post_sel_out o = out ? *out : evoamd_ais_post_sel_out{};
  AisPostPlan p;
  TRY(ais_post_plan(c, n_chains, n_temps, n_keep, betas, block_datapoints, flags, o.post.mean != nullptr, p, /*sel=*/true, index,
                    n_index, Mprime));
  if (o.admit_sums) o.admit_sums[0] = o.admit_sums[1] = 0.0;
  if (p.n == 0) return 0;  // an empty list: nothing to run, nothing written
  HIP_TRY(hipSetDevice(c->device));
  TRY(ais_post_prepare(c, p));
  TRY(ais_post_chains_stage(c, p, betas, seed, first_index, o.post.rb, index));
  if (p.mean) TRY(ais_post_mean_stage(c, p));
  if (p.admit) {
    double sums[2] = {0.0, 0.0};
    TRY(ais_post_admit_stage(c, p, Mprime, sums));
    if (o.admit_sums) o.admit_sums[0] = sums[0], o.admit_sums[1] = sums[1];
    const AisPostBufs b = ais_post_views(c, p);
    const size_t n = (size_t)p.n;
    HIP_TRY(fetch_if(c, o.F_before, b.F_before, n * sizeof(double)));
    HIP_TRY(fetch_if(c, o.F_after, b.F_after, n * sizeof(double)));
    HIP_TRY(fetch_if(c, o.n_distinct, b.n_distinct, n * sizeof(int)));
    HIP_TRY(fetch_if(c, o.n_new, b.n_new, n * sizeof(int)));
    HIP_TRY(fetch_if(c, o.n_proposed, b.n_proposed, n * sizeof(int)));
    HIP_TRY(fetch_if(c, o.n_admitted, b.n_admitted, n * sizeof(int)));
    HIP_TRY(fetch_if(c, o.map_held_before, b.held_before, n * sizeof(int)));
    HIP_TRY(fetch_if(c, o.map_held_after, b.held_after, n * sizeof(int)));
  }
  return ais_post_fetch(c, p, o.post);
}

// TEST-ONLY: the emission kernel alone on the caller's best_lpj (n, C) and best (n, C, HW words in the layout of K^n) for
// the rows `index` (n_index of them; NULL: the N datapoints), against the resident K^n.  The result is the candidate batch
// -- evaluated like any installed batch, so that evoamd_download_candidates reads it -- with the four count arrays (n
// each) and, where digests are in use, the digests written beside the candidates (N, Cmax; rows beyond a count are not
// written); *dig_used says whether.  Ties, non-finite values and duplicates cannot be had from the chains at will.
extern "C" int evoamd_ais_post_admit_probe(evoamd_ctx *c, const double *best_lpj, const uint64_t *best, int n_chains,
                                           const int64_t *index, int64_t n_index, int32_t *n_distinct, int32_t *n_new,
                                           int32_t *n_proposed, int32_t *map_held, uint64_t *dig_out, int *dig_used) {
  REQUIRE(c && c->configured, "configure first");
  REQUIRE(best_lpj && best && n_distinct && n_new && n_proposed && map_held, "evoamd_ais_post_admit_probe: bad arguments");
  REQUIRE(c->have_params && c->have_data, "evoamd_ais_post_admit_probe: Theta and data first (the batch is evaluated)");
  REQUIRE(n_chains >= 1, "evoamd_ais_post_admit_probe: n_chains must be positive");
  REQUIRE_KN(c);
  TRY(ais_post_check_index(c, "evoamd_ais_post_admit_probe", index, n_index));
  AisPostPlan p;
  p.C = n_chains, p.listed = index != nullptr, p.n = p.listed ? n_index : c->N, p.admit = true;
  const size_t n = (size_t)p.n, NC = n * (size_t)n_chains;
  HIP_TRY(hipSetDevice(c->device));
  TRY(c->aisp_d.ensure(c, 1 + 3 * NC + 2 * n * c->H + 9 * n + (size_t)c->N));
  TRY(c->aisp_i.ensure(c, 2 * NC + 6 * n + 1));
  TRY(c->aisp_s.ensure(c, NC * c->HW + n * c->HW + 1));
  TRY(c->aisp_nf.ensure(c, 2 * n + 1));
  const AisPostBufs b = ais_post_views(c, p);
  HIP_TRY(hipMemcpyAsync(b.best_lpj, best_lpj, NC * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(b.best, best, NC * c->HW * sizeof(u64), hipMemcpyHostToDevice, c->stream));
  if (p.listed && n) HIP_TRY(hipMemcpyAsync(b.index, index, n * sizeof(i64), hipMemcpyHostToDevice, c->stream));
  AisPostAdmitArgs a = ais_post_admit_args(c, p, b);
  a.map_held = b.held_before;
  TRY(ais_post_emit(c, a));
  on_cand_installed(c, /*near_parents=*/false);
  TRY(eval_candidates(c));
  made_cand_lpj(c);
  HIP_TRY(fetch_if(c, n_distinct, b.n_distinct, n * sizeof(int)));
  HIP_TRY(fetch_if(c, n_new, b.n_new, n * sizeof(int)));
  HIP_TRY(fetch_if(c, n_proposed, b.n_proposed, n * sizeof(int)));
  HIP_TRY(fetch_if(c, map_held, b.held_before, n * sizeof(int)));
  if (dig_used) *dig_used = a.cand_dig ? 1 : 0;
  if (a.cand_dig) HIP_TRY(fetch_if(c, dig_out, a.cand_dig, (size_t)c->N * c->Cmax * sizeof(u64)));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// posterior samples (kernels_posterior_sample.hpp): own buffers; of the EM state only B = Y W is (re)formed, like every lpj pass
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_posterior_sample(evoamd_ctx *c, int n_samples, uint64_t seed, uint64_t first_index, int keep_mask,
                                       int fill_all, int add_noise, int64_t counters[4]) {
  TRY(readout_admit(c, "evoamd_posterior_sample"));
  REQUIRE(counters, "evoamd_posterior_sample: counters is NULL");
  REQUIRE(n_samples >= 1, "evoamd_posterior_sample: n_samples must be positive");
  const bool sssc = c->model == EVOAMD_MODEL_SSSC;
  const int all = PSAMP_KEEP_SLOT | PSAMP_KEEP_S | PSAMP_KEEP_Z | PSAMP_KEEP_Y;
  REQUIRE(keep_mask != 0 && (keep_mask & ~all) == 0, "evoamd_posterior_sample: keep_mask must name at least one of the outputs (bits 1, 2, 4, 8)");
  REQUIRE(sssc || !(keep_mask & PSAMP_KEEP_Z), "evoamd_posterior_sample: z is an ES3C output (EBSC: z = s)");
  TRY(pred_admit_D(c, "evoamd_posterior_sample"));
  HIP_TRY(hipSetDevice(c->device));
  const i64 N = c->N, T = n_samples;
  const int D = c->D, H = c->H, HW = c->HW;
  made_posterior_samples(c, -1);
  // ---- do the outputs fit?  Decided before anything is released, allocated or launched.
  const size_t nt = (size_t)N * (size_t)T;
  FitList outputs;
  if (keep_mask & PSAMP_KEEP_SLOT) outputs.add(c->ps_slot, nt);
  if (keep_mask & PSAMP_KEEP_S) outputs.add(c->ps_s, nt * HW);
  if (keep_mask & PSAMP_KEEP_Z) outputs.add(c->ps_z, nt * H);
  if (keep_mask & PSAMP_KEEP_Y) outputs.add(c->ps_y, nt * D);
  outputs.add(c->ps_status, (size_t)N);
  outputs.add(c->pred_Wt, (size_t)H * D);
  size_t avail;
  TRY(outputs.measure(avail));
  if (outputs.grow > avail)
    return fail(EVOAMD_E_INVALID, "evoamd_posterior_sample: the outputs asked for need %zu bytes of device memory, %zu are free "
                "(fewer draws per call, or fewer arrays in keep)", outputs.grow, avail);
  if (sssc) TRY(ensure_B(c));
  TRY(outputs.ensure_all(c));
  double dpar[DP_COUNT];
  HIP_TRY(hipMemcpyAsync(dpar, c->dpar, DP_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  PsampArgs q = {};
  PredArgs &a = q.p;
  const PredLaunch l = fill_pred_args(c, a);
  q.sigma = pred_sigma(c, dpar, a);
  a.status = c->ps_status;
  q.Y = c->Y;
  q.ldY = c->ldY;
  q.T = T;
  q.seed = seed, q.first_index = first_index;
  q.fill_all = fill_all ? 1 : 0, q.add_noise = add_noise ? 1 : 0;
  q.slot = (keep_mask & PSAMP_KEEP_SLOT) ? c->ps_slot.get() : nullptr;
  q.s = (keep_mask & PSAMP_KEEP_S) ? c->ps_s.get() : nullptr;
  q.z = (keep_mask & PSAMP_KEEP_Z) ? c->ps_z.get() : nullptr;
  q.y = (keep_mask & PSAMP_KEEP_Y) ? c->ps_y.get() : nullptr;
  {
    SpanGuard g(c, KID_POSTERIOR_SAMPLE);
    pred_transpose_W(c);
    pred_dispatch(l.R, sssc, [&](auto r, auto s) {
      posterior_sample_kernel<decltype(r)::value, decltype(s)::value><<<cdiv(N, PRED_WAVES), 64 * PRED_WAVES, l.lds, c->stream>>>(q);
    });
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "posterior_sample");
  std::vector<int> status((size_t)N);
  HIP_TRY(hipMemcpyAsync(status.data(), c->ps_status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  TRY(pred_tally("evoamd_posterior_sample", status.data(), N, counters, {PSAMP_NOT_PD, PSAMP_BAD_WEIGHTS}));
  c->ps_N = N, c->ps_T = T, c->ps_D = D, c->ps_H = H;
  made_posterior_samples(c, keep_mask);
  return 0;
}

extern "C" int evoamd_download_posterior_samples(evoamd_ctx *c, int what, void *out) {
  REQUIRE(c && out, "evoamd_download_posterior_samples: NULL argument");
  REQUIRE(c->configured && c->ps_keep >= 0 && c->ps_N == c->N && c->ps_D == c->D && c->ps_H == c->H,
          "evoamd_download_posterior_samples: no results on the device (call evoamd_posterior_sample first; a failed call and "
          "evoamd_configure drop them)");
  const size_t nt = (size_t)c->ps_N * (size_t)c->ps_T;
  const void *src = nullptr;
  size_t bytes = 0;
  int bit = 0;
  switch (what) {
    case EVOAMD_PSAMP_SLOT: src = c->ps_slot, bytes = nt * sizeof(int), bit = PSAMP_KEEP_SLOT; break;
    case EVOAMD_PSAMP_S: src = c->ps_s, bytes = nt * c->HW * sizeof(u64), bit = PSAMP_KEEP_S; break;
    case EVOAMD_PSAMP_Z: src = c->ps_z, bytes = nt * c->ps_H * sizeof(double), bit = PSAMP_KEEP_Z; break;
    case EVOAMD_PSAMP_Y: src = c->ps_y, bytes = nt * c->ps_D * sizeof(double), bit = PSAMP_KEEP_Y; break;
    default: return fail(EVOAMD_E_INVALID, "evoamd_download_posterior_samples: what must be EVOAMD_PSAMP_SLOT, _S, _Z or _Y");
  }
  REQUIRE(c->ps_keep & bit, "evoamd_download_posterior_samples: the last evoamd_posterior_sample did not keep this output");
  return download_view(c, out, src, bytes);
}

// ---------------------------------------------------------------------------------------
// log-likelihood beyond K^n by importance draws (kernels_loglik_estimate.hpp).  The outside draws of a pass go through
// the RESIDENT CANDIDATE BATCH (c->cand, cand_dig, cand_counts, cand_lpj) and eval_candidates' launches under tag 1, not
// through a private batch under tag 2: the candidate instantiations are the ones built for ragged per-datapoint states at
// the large shapes (EBSC: the Gram form over B = Y W instead of the direct residual; ES3C: the table-driven main kernel
// over digests, which dig_for only grants the two resident arrays), a pass is then at most Cmax draws by construction and
// no second N x Cmax x HW array exists.  The price: the batch a previous E-step left is gone (drop_cand_batch), and the
// hints say "nothing known" (known_tag 2: every level, worst-case grids), because draws are no children of K^n.  The clamp
// flags go to words of the call's own, so the reset counters of the next evoamd_stats do not see the draws.
// ---------------------------------------------------------------------------------------
static int lle_kh(int HW) { return HW <= 1 ? 1 : HW <= 2 ? 2 : HW <= 4 ? 4 : HW <= 8 ? 8 : LLE_MAX_KH; }  // latents per lane

static void launch_lle_proposal(evoamd_ctx *c, const LleArgs &a, size_t lds) {
  const unsigned grid = cdiv(a.N, LLE_WAVES);
  switch (lle_kh(a.HW)) {  // (a.rho holds N x 64 lle_kh(HW) doubles)
    case 1: lle_proposal_kernel<1><<<grid, 64 * LLE_WAVES, lds, c->stream>>>(a); break;
    case 2: lle_proposal_kernel<2><<<grid, 64 * LLE_WAVES, lds, c->stream>>>(a); break;
    case 4: lle_proposal_kernel<4><<<grid, 64 * LLE_WAVES, lds, c->stream>>>(a); break;
    case 8: lle_proposal_kernel<8><<<grid, 64 * LLE_WAVES, lds, c->stream>>>(a); break;
    default: lle_proposal_kernel<LLE_MAX_KH><<<grid, 64 * LLE_WAVES, lds, c->stream>>>(a); break;
  }
}

// Plan (every refusal that reads the arguments and the geometry, the sizes), then the named stages: prepare (with the one
// refusal that needs the device: do the buffers fit?), the passes (proposal -> candidate lpj -> fold), finish, fetch.
struct LlePlan {
  bool sssc = false, keep = false;
  i64 T = 0;
  int Hv = 0;  // latents that vary
  double lam = 0.0;
  unsigned nb = 1;                           // workgroups of the fold and the finish
  size_t lds = 0, nt = 0;                    // LDS of the proposal kernel; N x T
  size_t n_d = 0, n_i = 0, n_rho = 0;        // elements of lle_d / lle_i / lle_rho
};

static int lle_plan(const evoamd_ctx *c, int n_samples, double prior_mix, int keep_draws, const int64_t *counters,
                    const double *sum_out, LlePlan &p) {
  TRY(readout_admit(c, "evoamd_loglik_estimate"));
  REQUIRE(counters && sum_out, "evoamd_loglik_estimate: counters or sum_out is NULL");
  REQUIRE(n_samples >= 1, "evoamd_loglik_estimate: n_samples must be positive");
  REQUIRE(prior_mix > 0.0 && prior_mix <= 1.0, "evoamd_loglik_estimate: prior_mix must be in (0, 1]");
  p.sssc = c->model == EVOAMD_MODEL_SSSC, p.keep = keep_draws != 0;
  p.T = n_samples, p.Hv = c->H - (c->bg_unit ? 1 : 0), p.lam = prior_mix;
  if (c->HW > LLE_MAX_KH)
    return fail(EVOAMD_E_INVALID, "evoamd_loglik_estimate: H = %d, at most %d latents are supported (64 lanes x %d registers)", c->H,
                64 * LLE_MAX_KH, LLE_MAX_KH);
  REQUIRE(p.Hv >= 1, "evoamd_loglik_estimate: no latent varies");
  p.lds = (size_t)LLE_WAVES * (size_t)(c->L + c->S) * sizeof(double);
  if (p.lds > LLE_LDS_MAX)
    return fail(EVOAMD_E_INVALID, "evoamd_loglik_estimate: S_perm + 2 S = %d, at most %d weights and hashes fit the LDS slice of a "
                "datapoint", c->L + c->S, (int)(LLE_LDS_MAX / (LLE_WAVES * sizeof(double))));
  const size_t N = (size_t)c->N, nc = N * (size_t)c->Cmax;
  p.nt = N * (size_t)p.T;
  p.nb = cdiv(c->N, 4);
  p.n_d = 8 * N + 1 + p.nb + nc;  // F | m | z | q | ll | mass | ess | all-zero lpj (N each) | sum (1) | partial (nb) | log r (N x Cmax)
  p.n_i = 2 * N + nc;             // status | n_outside | t (N x Cmax)
  p.n_rho = N * 64 * (size_t)lle_kh(c->HW);
  return 0;
}

// the views into the call's buffers
struct LleBufs {
  double *F, *run_m, *run_z, *run_q, *ll, *mass, *ess, *az, *sum, *part, *logr, *keep_logr, *keep_lpj;
  int *status, *n_out, *tix;
};
static LleBufs lle_views(const evoamd_ctx *c, const LlePlan &p) {
  const size_t N = (size_t)c->N;
  LleBufs b;
  b.F = c->lle_d, b.run_m = b.F + N, b.run_z = b.run_m + N, b.run_q = b.run_z + N, b.ll = b.run_q + N, b.mass = b.ll + N;
  b.ess = b.mass + N, b.az = b.ess + N, b.sum = b.az + N, b.part = b.sum + 1, b.logr = b.part + p.nb;
  b.status = c->lle_i, b.n_out = b.status + N, b.tix = b.n_out + N;
  b.keep_logr = p.keep ? c->lle_keep_d.get() : nullptr, b.keep_lpj = p.keep ? b.keep_logr + p.nt : nullptr;
  return b;
}

// ---- stage: every buffer (do they fit?  Decided before anything is released, allocated or launched), the candidate batch
// given up, F of K^n and the lpj of the all-zero state
static int lle_prepare(evoamd_ctx *c, const LlePlan &p) {
  const size_t N = (size_t)c->N;
  FitList bufs;
  bufs.add(c->lle_d, p.n_d), bufs.add(c->lle_i, p.n_i), bufs.add(c->lle_flags, N);
  bufs.add(c->lle_rho, p.n_rho), bufs.add(c->lle_hash, N * c->S);
  if (p.keep) bufs.add(c->lle_keep_s, p.nt * c->HW), bufs.add(c->lle_keep_in, p.nt), bufs.add(c->lle_keep_d, 2 * p.nt);
  size_t avail;
  TRY(bufs.measure(avail));
  if (bufs.grow > avail)
    return fail(EVOAMD_E_INVALID, "evoamd_loglik_estimate: the buffers asked for need %zu bytes of device memory, %zu are free "
                "(fewer draws per call, or keep_draws = 0)", bufs.grow, avail);
  TRY(ensure_B(c));
  if (p.sssc) TRY(ensure_lists(c, c->N * (i64)c->Cmax));
  TRY(bufs.ensure_all(c));
  if (p.keep) {
    // a datapoint without an estimate keeps these: s zero, inside 0, log r and lpj NaN (all bits set); so does the lpj
    // of an inside draw
    HIP_TRY(hipMemsetAsync(c->lle_keep_s, 0, p.nt * c->HW * sizeof(u64), c->stream));
    HIP_TRY(hipMemsetAsync(c->lle_keep_in, 0, p.nt, c->stream));
    HIP_TRY(hipMemsetAsync(c->lle_keep_d, 0xFF, 2 * p.nt * sizeof(double), c->stream));
  }
  HIP_TRY(hipMemsetAsync(c->lle_flags, 0, N * sizeof(unsigned), c->stream));
  const LleBufs b = lle_views(c, p);
  drop_cand_batch(c);  // from here on the candidate buffers hold importance draws
  SpanGuard g(c, KID_LLE_FOLD);
  posterior_score_kernel<<<cdiv(c->N, SCORE_WAVES), 64 * SCORE_WAVES, 0, c->stream>>>(c->lpj, c->states, c->N, c->L, c->S, c->S_perm,
                                                                                      c->HW, b.F, nullptr, nullptr, nullptr, nullptr);
  allzero_lpj_kernel<<<cdiv(c->N, 256), 256, 0, c->stream>>>(c->yy, c->N, c->dpar, p.sssc, b.az, 1, c->lle_flags, c->err);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- stage: the passes of at most Cmax draws each: proposal -> lpj of the outside draws -> fold
static int lle_passes_stage(evoamd_ctx *c, const LlePlan &p, uint64_t seed, uint64_t first_index) {
  const LleBufs b = lle_views(c, p);
  const i64 N = c->N;
  const int Cmax = c->Cmax;
  LleArgs a = {};
  a.lpj = c->lpj, a.states = c->states;
  a.pies = p.sssc ? c->pies.get() : nullptr;
  a.dpar = c->dpar;
  a.row_any = c->mask_infr ? c->row_any.get() : nullptr;
  a.N = N, a.T = p.T;
  a.H = c->H, a.Hv = p.Hv, a.HW = c->HW, a.S = c->S, a.S_perm = c->S_perm, a.L = c->L, a.bg = c->bg_unit ? 1 : 0, a.Cmax = Cmax;
  a.lam = p.lam, a.oml = 1.0 - p.lam;
  a.seed = seed, a.first_index = first_index;
  a.cand = c->cand, a.cand_dig = (c->use_digest && c->cand_dig) ? c->cand_dig.get() : nullptr, a.counts = c->cand_counts;
  a.logr = b.logr, a.tix = b.tix, a.status = b.status, a.rho = c->lle_rho, a.hash = c->lle_hash;
  a.keep_s = p.keep ? c->lle_keep_s.get() : nullptr;
  a.keep_inside = p.keep ? c->lle_keep_in.get() : nullptr;
  a.keep_logr = b.keep_logr;
  const LevelHints lv;  // known_tag 2: nothing is known about the draws
  for (i64 t0 = 0; t0 < p.T; t0 += Cmax) {
    a.t0 = t0;
    a.P = (int)std::min<i64>(Cmax, p.T - t0);
    {
      SpanGuard g(c, KID_LLE_PROPOSAL);
      launch_lle_proposal(c, a, p.lds);
      HIP_TRY(hipGetLastError());
      DBG_SYNC(c, "loglik_estimate proposal");
    }
    on_cand_installed(c, /*near_parents=*/false);
    {
      SpanGuard g(c, KID_LLE_LPJ);
      Batch bt = {c->cand, c->cand_counts, c->Y, c->Bm, c->yy, N, Cmax, 0, c->cand_lpj, Cmax, 0, c->lle_flags, KID_LPJ_CAND, 1};
      bt.mask = c->mask_infr;
      TRY(launch_lpj(c, bt, lv));
    }
    SpanGuard g(c, KID_LLE_FOLD);
    lle_fold_kernel<<<p.nb, 256, 0, c->stream>>>(c->cand_lpj, Cmax, c->cand_counts, b.logr, b.tix, b.az, N, p.T, t0 == 0, b.run_m,
                                                 b.run_z, b.run_q, b.n_out, b.keep_lpj);
    HIP_TRY(hipGetLastError());
    DBG_SYNC(c, "loglik_estimate fold");
  }
  return 0;
}

// ---- stage: the estimate of every datapoint and their sum
static int lle_finish_stage(evoamd_ctx *c, const LlePlan &p) {
  const LleBufs b = lle_views(c, p);
  SpanGuard g(c, KID_LLE_FOLD);
  lle_finish_kernel<<<p.nb, 256, 0, c->stream>>>(b.F, b.run_m, b.run_z, b.run_q, b.n_out, b.status, c->N, log((double)p.T), b.ll, b.mass,
                                                 b.ess, b.part);
  reduce_partials_kernel<<<1, 256, 0, c->stream>>>(b.part, p.nb, b.sum, 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- stage: the outputs, each where the caller gave a buffer; the counts of the datapoints without an estimate
static int lle_fetch(evoamd_ctx *c, const LlePlan &p, double *ll, double *F, double *mass, double *ess, int32_t *n_outside,
                     int64_t counters[2], double *sum) {
  const LleBufs b = lle_views(c, p);
  const size_t N = (size_t)c->N;
  std::vector<int> status(N);
  HIP_TRY(hipMemcpyAsync(status.data(), b.status, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(fetch_if(c, ll, b.ll, N * sizeof(double)));
  HIP_TRY(fetch_if(c, F, b.F, N * sizeof(double)));
  HIP_TRY(fetch_if(c, mass, b.mass, N * sizeof(double)));
  HIP_TRY(fetch_if(c, ess, b.ess, N * sizeof(double)));
  HIP_TRY(fetch_if(c, n_outside, b.n_out, N * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(sum, b.sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (p.sssc)
    TRY(check_err(c));  // synchronises the stream; a draw the levels refuse surfaces here
  else
    HIP_TRY(hipStreamSynchronize(c->stream));
  counters[0] = counters[1] = 0;
  for (size_t n = 0; n < N; n++) counters[0] += status[n] == LLE_BAD_WEIGHTS, counters[1] += status[n] == LLE_SKIPPED;
  return 0;
}

extern "C" int evoamd_loglik_estimate(evoamd_ctx *c, int n_samples, uint64_t seed, uint64_t first_index, double prior_mix,
                                      int keep_draws, double *ll_out, double *F_out, double *mass_out, double *ess_out,
                                      int32_t *n_outside_out, int64_t counters[2], double *sum_out) {
  LlePlan p;
  TRY(lle_plan(c, n_samples, prior_mix, keep_draws, counters, sum_out, p));
  HIP_TRY(hipSetDevice(c->device));
  made_loglik_draws(c, -1);
  TRY(lle_prepare(c, p));
  TRY(lle_passes_stage(c, p, seed, first_index));
  TRY(lle_finish_stage(c, p));
  TRY(lle_fetch(c, p, ll_out, F_out, mass_out, ess_out, n_outside_out, counters, sum_out));
  c->lle_N = c->N, c->lle_T = p.T, c->lle_H = c->H;
  made_loglik_draws(c, p.keep ? 1 : 0);
  return 0;
}

extern "C" int evoamd_download_loglik_draws(evoamd_ctx *c, int what, void *out) {
  REQUIRE(c && out, "evoamd_download_loglik_draws: NULL argument");
  REQUIRE(c->configured && c->lle_keep == 1 && c->lle_N == c->N && c->lle_H == c->H,
          "evoamd_download_loglik_draws: no draws on the device (call evoamd_loglik_estimate with keep_draws first; a failed "
          "call and evoamd_configure drop them)");
  const size_t nt = (size_t)c->lle_N * (size_t)c->lle_T;
  const void *src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case EVOAMD_LLE_S: src = c->lle_keep_s, bytes = nt * c->HW * sizeof(u64); break;
    case EVOAMD_LLE_INSIDE: src = c->lle_keep_in, bytes = nt; break;
    case EVOAMD_LLE_LOG_R: src = c->lle_keep_d, bytes = nt * sizeof(double); break;
    case EVOAMD_LLE_LPJ: src = c->lle_keep_d + nt, bytes = nt * sizeof(double); break;
    default: return fail(EVOAMD_E_INVALID, "evoamd_download_loglik_draws: what must be EVOAMD_LLE_S, _INSIDE, _LOG_R or _LPJ");
  }
  return download_view(c, out, src, bytes);
}

// ---------------------------------------------------------------------------------------
// samples from the model (kernels_generate.hpp): own buffers, no EM state touched
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_generate(evoamd_ctx *c, int model, int64_t N, int D, int H, uint64_t seed, uint64_t first_index,
                               const double *Wt, const double *pies, const double *mus, const double *F, double sigma,
                               const uint64_t *s_packed, int keep) {
  REQUIRE(c && Wt && pies, "evoamd_generate: NULL argument");
  REQUIRE(model == EVOAMD_MODEL_BSC || model == EVOAMD_MODEL_SSSC, "evoamd_generate: model must be EVOAMD_MODEL_BSC or EVOAMD_MODEL_SSSC");
  REQUIRE(N >= 1 && D >= 1 && H >= 1, "evoamd_generate: N, D and H must be positive");
  REQUIRE(sigma >= 0.0 && sigma <= 1.7976931348623157e308, "evoamd_generate: sigma must be finite and not negative");
  REQUIRE((keep & ~(EVOAMD_GEN_KEEP_S | EVOAMD_GEN_KEEP_Z | EVOAMD_GEN_KEEP_YMEAN)) == 0, "evoamd_generate: unknown bit in keep");
  const bool sssc = model == EVOAMD_MODEL_SSSC;
  REQUIRE(!sssc || (mus && F), "evoamd_generate: ES3C needs mus and F (F F^T = Psi)");
  if (!sssc) keep &= ~EVOAMD_GEN_KEEP_Z;  // EBSC: z = s
  const size_t slice = sssc ? (size_t)H * sizeof(double) : 0;
  if (slice > 64 * 1024)
    return fail(EVOAMD_E_INVALID, "evoamd_generate: the eps values of one datapoint (H = %d doubles) exceed the 64 KB of LDS a wavefront may hold", H);
  HIP_TRY(hipSetDevice(c->device));
  const int HW = (H + 63) / 64;
  const size_t nd = (size_t)N * D, nh = (size_t)N * H, nw = (size_t)N * HW;
  const size_t par_n = (size_t)H * D + H + (sssc ? (size_t)H + (size_t)H * H : 0);
  made_generated(c, -1);  // until this call has completed
  TRY(c->gen_par.ensure(c, par_n));
  TRY(c->gen_y.ensure(c, nd));
  if (keep & EVOAMD_GEN_KEEP_S) TRY(c->gen_s.ensure(c, nw));
  if (keep & EVOAMD_GEN_KEEP_Z) TRY(c->gen_z.ensure(c, nh));
  if (keep & EVOAMD_GEN_KEEP_YMEAN) TRY(c->gen_ymean.ensure(c, nd));
  if (s_packed) TRY(c->gen_sin.ensure(c, nw));
  double *dWt = c->gen_par, *dpies = dWt + (size_t)H * D, *dmus = dpies + H, *dF = dmus + H;
  HIP_TRY(hipMemcpyAsync(dWt, Wt, (size_t)H * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(dpies, pies, (size_t)H * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (sssc) {
    HIP_TRY(hipMemcpyAsync(dmus, mus, (size_t)H * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dF, F, (size_t)H * H * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (s_packed) HIP_TRY(hipMemcpyAsync(c->gen_sin, s_packed, nw * sizeof(u64), hipMemcpyHostToDevice, c->stream));
  GenArgs a;
  a.Wt = dWt;
  a.pies = dpies;
  a.mus = sssc ? dmus : nullptr;
  a.F = sssc ? dF : nullptr;
  a.s_in = s_packed ? c->gen_sin : nullptr;
  a.y = c->gen_y;
  a.s_out = (keep & EVOAMD_GEN_KEEP_S) ? c->gen_s : nullptr;
  a.z = (keep & EVOAMD_GEN_KEEP_Z) ? c->gen_z : nullptr;
  a.y_mean = (keep & EVOAMD_GEN_KEEP_YMEAN) ? c->gen_ymean : nullptr;
  a.N = N;
  a.D = D;
  a.H = H;
  a.HW = HW;
  a.sssc = sssc ? 1 : 0;
  a.seed = seed;
  a.first_index = first_index;
  a.sigma = sigma;
  int W = 4;  // waves per workgroup: their eps slices share 64 KB
  while (W > 1 && W * slice > 64 * 1024) W >>= 1;
  const unsigned grid = (unsigned)std::min<i64>(cdiv(N, W), (i64)c->n_cu * 64);
  {
    SpanGuard g(c, KID_MISC);
    generate_kernel<<<grid, 64 * W, W * slice, c->stream>>>(a);
  }
  HIP_TRY(hipGetLastError());
  DBG_SYNC(c, "generate");
  HIP_TRY(hipStreamSynchronize(c->stream));  // the host arrays are borrowed for the call only
  c->gen_N = N;
  c->gen_D = D;
  c->gen_H = H;
  made_generated(c, keep);
  return 0;
}

extern "C" int evoamd_download_generated(evoamd_ctx *c, int what, void *out) {
  REQUIRE(c && out, "evoamd_download_generated: NULL argument");
  REQUIRE(c->gen_keep >= 0, "evoamd_download_generated: no evoamd_generate call has completed");
  const size_t nd = (size_t)c->gen_N * c->gen_D * sizeof(double);
  const void *src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case EVOAMD_GEN_Y: src = c->gen_y, bytes = nd; break;
    case EVOAMD_GEN_S:
      REQUIRE(c->gen_keep & EVOAMD_GEN_KEEP_S, "evoamd_download_generated: s was not kept by the last evoamd_generate (keep bit 1)");
      src = c->gen_s, bytes = (size_t)c->gen_N * ((c->gen_H + 63) / 64) * sizeof(u64);
      break;
    case EVOAMD_GEN_Z:
      REQUIRE(c->gen_keep & EVOAMD_GEN_KEEP_Z, "evoamd_download_generated: z was not kept by the last evoamd_generate (keep bit 2, ES3C only)");
      src = c->gen_z, bytes = (size_t)c->gen_N * c->gen_H * sizeof(double);
      break;
    case EVOAMD_GEN_YMEAN:
      REQUIRE(c->gen_keep & EVOAMD_GEN_KEEP_YMEAN, "evoamd_download_generated: y_mean was not kept by the last evoamd_generate (keep bit 4)");
      src = c->gen_ymean, bytes = nd;
      break;
    default: return fail(EVOAMD_E_INVALID, "evoamd_download_generated: what must be EVOAMD_GEN_Y, _S, _Z or _YMEAN");
  }
  return download_view(c, out, src, bytes);
}

// ---------------------------------------------------------------------------------------
// RCCL
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_comm_unique_id(uint8_t id_out[128]) {
  TRY(rccl_load());
  RcclId id;
  RCCL_TRY(g_rccl.GetUniqueId(&id));
  memcpy(id_out, id.internal, 128);
  return 0;
}

extern "C" int evoamd_comm_init(evoamd_ctx *c, const uint8_t id_in[128], int rank, int world) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
  TRY(rccl_load());
  HIP_TRY(hipSetDevice(c->device));
  RcclId id;
  memcpy(id.internal, id_in, 128);
  RCCL_TRY(g_rccl.CommInitRank(&c->comm, world, id, rank));
  c->pays_agreed = -1;
  c->rank = rank;
  c->world = world;
  return 0;
}

extern "C" int evoamd_comm_allreduce_host(evoamd_ctx *c, double *buf, int64_t n, int op) {
  REQUIRE(c && buf && n > 0, "bad arguments");
  if (!c->comm) return 0;  // single rank: identity
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<double> d;
  TRY(d.alloc((size_t)n));
  HIP_TRY(hipMemcpyAsync(d, buf, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int rc = g_rccl.AllReduce(d, d, (size_t)n, 8, op == 1 ? 2 : 0, c->comm, c->stream);
  if (rc != 0) return fail(EVOAMD_E_RCCL, "ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
  HIP_TRY(hipMemcpyAsync(buf, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int evoamd_comm_destroy(evoamd_ctx *c) {
  REQUIRE(c, "ctx is NULL");
  if (c->comm) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    RCCL_TRY(g_rccl.CommDestroy(c->comm));
    c->comm = nullptr;
    c->world = 1;
    c->rank = 0;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------------------
extern "C" int evoamd_timing_enable(evoamd_ctx *c, int on) {
  REQUIRE(c, "ctx is NULL");
  if (!on && c->timing) TRY(resolve_spans(c));
  c->timing = on != 0;
  c->timing_mask = (u64)(i64)on;  // bit k = kernel class k; -1 reaches the classes from 32 on too
  return 0;
}

extern "C" int evoamd_timing_enable64(evoamd_ctx *c, uint64_t on) {
  REQUIRE(c, "ctx is NULL");
  if (!on && c->timing) TRY(resolve_spans(c));
  c->timing = on != 0;
  c->timing_mask = on;  // bit k = kernel class k; 1-bits beyond EVOAMD_K_COUNT are harmless
  return 0;
}

extern "C" int evoamd_timing_reset(evoamd_ctx *c) {
  REQUIRE(c, "ctx is NULL");
  TRY(resolve_spans(c));
  for (int i = 0; i < KID_COUNT; i++) {
    c->t_ms[i] = 0;
    c->t_n[i] = 0;
  }
  return 0;
}

extern "C" int evoamd_kernel_time_ms(evoamd_ctx *c, int kid, double *avg_ms, int64_t *launches) {
  REQUIRE(c && kid >= 0 && kid < KID_COUNT, "bad kernel id");
  TRY(resolve_spans(c));
  if (avg_ms) *avg_ms = c->t_n[kid] ? c->t_ms[kid] / (double)c->t_n[kid] : 0.0;
  if (launches) *launches = c->t_n[kid];
  return 0;
}

extern "C" const char *evoamd_kernel_name(int kid) {
  static const char *names[KID_COUNT] = {"lpj_resident", "lpj_candidates", "lpj_overflow", "row_lse",  "vary_kn",
                                         "stats",        "stats_overflow", "gemm_f64",     "evolve",   "misc", "mstep_device",
                                         "lpj_pass",     "stats_pass",     "lpj_k3_4",     "lpj_k5_8", "lpj_k9plus",
                                         "stats_k3_4",   "stats_k5_8",     "stats_k9plus", "allreduce",    "estep_fused",
                                         "patches",      "init_states",    "posterior_sample", "seed_states",
                                         "loglik_proposal", "loglik_lpj",  "loglik_fold",     "remap_latents",
                                         "stats_kappa",  "sweep",       "sweep_swap",      "resize",
                                         "neighbour_bound", "predictive_score",
                                         "ais",          "ais_post"};
  return (kid >= 0 && kid < KID_COUNT) ? names[kid] : "?";
}
