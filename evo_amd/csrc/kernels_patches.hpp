// Overlapping image patches: extract an image into patch rows and merge patch rows back into an image by the mean or
// the median of every pixel's estimates (the image workflows of the reference's examples: image-denoising /
// image-inpainting main.py, OverlappingPatches.get / set_and_merge with mean_merger / median_merger).
//
// Conventions (ours; evo_amd/utils/prepost.py states the same):
//   image   f64 (H, W, C) row-major, C innermost (C = 1 for grey images).
//   tops    0, s, 2s, ... while <= H - ph, plus H - ph appended if that value was not reached (every pixel is covered);
//           lefts the same with W, pw.  Patch top of grid row i = min(i s, H - ph).
//   n       = ir * nc + ic, row-major over the (top row, left column) grid; N = nr * nc.
//   d       = (dy * pw + dx) * C + c; D = ph * pw * C.
//   mean    the covering estimates summed in increasing n (NaN skipped), divided by their count: bit-identical to
//           np.nanmean(stack, axis=0) over the NaN-padded (K, H, W[, C]) stack of estimates in increasing n (NumPy adds
//           the slices of axis 0 one after another).  Adds only: no contraction.
//   median  bit-identical to np.nanmedian(stack, axis=0): odd count -> the middle value, even -> (lo + hi) / 2.
//   no valid estimate -> NaN.
//   limits  ph pw <= 1024, ph <= H, pw <= W, s >= 1.
#pragma once
#include "common.hpp"

#define PATCH_MAX_ELEMS 1024  // ph * pw

struct PatchGeom {
  int H, W, C, ph, pw, s;
  int nr, nc;  // grid rows / columns
  int D;       // ph * pw * C
  i64 N;       // nr * nc
};

// patch tops along one axis of length L: ceil((L - p) / s) + 1 of them
__host__ __device__ __forceinline__ int patch_grid_count(int L, int p, int s) { return (L - p) / s + 1 + ((L - p) % s != 0); }
__host__ __device__ __forceinline__ int patch_top(int i, int L, int p, int s) {
  const int t = i * s;
  return t < L - p ? t : L - p;
}
// grid indices [lo, hi] of the patches covering coordinate y (tops strictly increase, so every index between covers)
__host__ __device__ __forceinline__ void patch_cover(int y, int L, int p, int s, int n, int &lo, int &hi) {
  const int a = y - p + 1;
  lo = a > 0 ? (a + s - 1) / s : 0;
  hi = y >= L - p ? n - 1 : y / s;
}

// Validates the arguments and fills g; returns NULL or a message.
static inline const char *patch_geom_make(int H, int W, int C, int ph, int pw, int s, PatchGeom *g) {
  if (H < 1 || W < 1 || C < 1) return "image dimensions H, W, C must be >= 1";
  if (ph < 1 || pw < 1) return "patch height and width must be >= 1";
  if (ph > H || pw > W) return "patch larger than the image (ph > H or pw > W)";
  if (s < 1) return "patch shift must be >= 1";
  if ((i64)ph * pw > PATCH_MAX_ELEMS) return "ph * pw > 1024 (patches above 32 x 32 elements are not supported)";
  if ((i64)ph * pw * C > (1 << 30)) return "ph * pw * C too large";
  g->H = H, g->W = W, g->C = C, g->ph = ph, g->pw = pw, g->s = s;
  g->nr = patch_grid_count(H, ph, s);
  g->nc = patch_grid_count(W, pw, s);
  g->D = ph * pw * C;
  g->N = (i64)g->nr * g->nc;
  return nullptr;
}

// Largest number of estimates of one pixel: (most covering rows) x (most covering columns).
static inline int patch_max_cover(const PatchGeom &g) {
  int kr = 0, kc = 0, lo, hi;
  for (int y = 0; y < g.H; y++) {
    patch_cover(y, g.H, g.ph, g.s, g.nr, lo, hi);
    kr = hi - lo + 1 > kr ? hi - lo + 1 : kr;
  }
  for (int x = 0; x < g.W; x++) {
    patch_cover(x, g.W, g.pw, g.s, g.nc, lo, hi);
    kc = hi - lo + 1 > kc ? hi - lo + 1 : kc;
  }
  return kr * kc;
}

// Y[n, d] = img[top + dy, left + dx, c]: one thread per element of Y (coalesced stores; the image is small and cached).
__global__ void __launch_bounds__(256) patches_extract_kernel(const double *__restrict__ img, PatchGeom g,
                                                              double *__restrict__ Y) {
  const i64 total = g.N * g.D;
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (i64)gridDim.x * blockDim.x) {
    const i64 n = e / g.D;
    const int d = (int)(e - n * g.D);
    const int ir = (int)(n / g.nc), ic = (int)(n - (i64)ir * g.nc);
    const int c = d % g.C, t = d / g.C;
    const int dy = t / g.pw, dx = t - dy * g.pw;
    const int y = patch_top(ir, g.H, g.ph, g.s) + dy, x = patch_top(ic, g.W, g.pw, g.s) + dx;
    Y[e] = img[((i64)y * g.W + x) * g.C + c];
  }
}

// Where the merge kernels read an estimate: element d of patch row n.
// PatchRows: a dense (N, D) matrix of patch rows.
struct PatchRows {
  const double *__restrict__ Y;
  __device__ __forceinline__ double load(i64 n, int d, int D) const { return Y[n * D + d]; }
  __device__ __forceinline__ i64 image() const { return 0; }  // which image of `out` this launch row (blockIdx.y) writes
};
// PatchDrawRows: the draws the last evoamd_posterior_sample kept, y (N, T, D), read where they lie: grid row blockIdx.y
// of a launch merges draw t0 + blockIdx.y into image blockIdx.y (one row: one draw).  The arithmetic of a merge of the
// dense (N, D) slice y[:, t, :], hence its bits; only the address differs.
struct PatchDrawRows {
  const double *__restrict__ y;
  i64 T;
  int t0;
  __device__ __forceinline__ double load(i64 n, int d, int D) const { return y[(n * T + t0 + blockIdx.y) * D + d]; }
  __device__ __forceinline__ i64 image() const { return blockIdx.y; }
};
// PatchSelect: the selected reconstruction of a configured context, formed while it is gathered (evoamd_reconstruct_resident):
//   complete data    x[n, d] ? Y[n, d] : y_hat[n, d]   (x == NULL: y_hat everywhere); rec = y_hat, infr == NULL
//   incomplete data  rec = y_reconstructed as select_rec_kernel left it for the M-step, in which a kept entry without a
//                    reliable value holds the 0 that mask_apply_kernel put into Y: it reads as NaN here (kept =
//                    x[n, d], or patch n has no reliable entry at all: any[n] == 0).  Precondition for parity with a
//                    merge of the host array: the caller's y is NaN wherever infr is 0 (evo_amd.h)
struct PatchSelect {
  const double *rec;    // (N, D)
  const double *Y;      // (N, ldY) resident data
  i64 ldY;
  const uint8_t *x;     // (N, D) keep-mask or NULL
  const uint8_t *infr;  // (N, D) reliable entries, NULL for complete data
  const uint8_t *any;   // (N) patch has a reliable entry (incomplete data)
  __device__ __forceinline__ double load(i64 n, int d, int D) const {
    const i64 e = n * D + d;
    if (infr) {
      const bool lost = !infr[e] && (x[e] || !any[n]);
      return lost ? __builtin_nan("") : rec[e];
    }
    return (x && x[e]) ? Y[n * ldY + d] : rec[e];
  }
  __device__ __forceinline__ i64 image() const { return 0; }
};

// The estimate of pixel (y, x, c) held by patch (ir, ic).
template <class Src>
__device__ __forceinline__ double patch_estimate(const Src &src, const PatchGeom &g, int ir, int ic, int y, int x, int c) {
  const int dy = y - patch_top(ir, g.H, g.ph, g.s), dx = x - patch_top(ic, g.W, g.pw, g.s);
  return src.load((i64)ir * g.nc + ic, (dy * g.pw + dx) * g.C + c, g.D);
}

// out[n, d] = src(n, d): the selected reconstruction written out as dense patch rows (the select-then-merge route of
// evoamd_patches_merge_resident; the fused route gathers through PatchSelect instead).
__global__ void __launch_bounds__(256) patches_select_kernel(PatchSelect src, i64 N, int D, double *__restrict__ out) {
  const i64 total = N * D;
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (i64)gridDim.x * blockDim.x) {
    const i64 n = e / D;
    out[e] = src.load(n, (int)(e - n * D), D);
  }
}

// any[n] = row n of the (N, D) byte mask has a non-zero entry; one wave per row.
__global__ void __launch_bounds__(256) patches_row_any_kernel(const uint8_t *__restrict__ mask, i64 N, int D,
                                                              uint8_t *__restrict__ any) {
  const int lane = lane_id();
  const i64 n = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (n >= N) return;
  bool a = false;
  for (int d = lane; d < D; d += 64) a = a || mask[n * D + d] != 0;
  a = __any(a);
  if (lane == 0) any[n] = a ? 1 : 0;
}

// Mean merge: one thread per output element, its estimates summed in increasing n (NumPy's order for axis 0).
template <class Src>
__global__ void __launch_bounds__(256) patches_mean_kernel(Src src, PatchGeom g, double *__restrict__ out) {
#pragma clang fp contract(off)
  const i64 total = (i64)g.H * g.W * g.C;
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % g.C);
  const i64 px = e / g.C;
  const int y = (int)(px / g.W), x = (int)(px - (i64)y * g.W);
  int r0, r1, c0, c1;
  patch_cover(y, g.H, g.ph, g.s, g.nr, r0, r1);
  patch_cover(x, g.W, g.pw, g.s, g.nc, c0, c1);
  double sum = 0.0;
  int cnt = 0;
  for (int ir = r0; ir <= r1; ir++)
    for (int ic = c0; ic <= c1; ic++) {
      const double v = patch_estimate(src, g, ir, ic, y, x, c);
      if (v == v) {
        sum += v;
        cnt++;
      }
    }
  out[src.image() * total + e] = cnt ? sum / (double)cnt : __builtin_nan("");
}

// Mean merge of draws t0 .. t0 + n - 1 of y (N, T, D) in one launch, and the pixelwise moments over the merged images.
// One thread per output element, as in patches_mean_kernel: the cover of the pixel is computed once for all draws, and the
// draws run one after the other in an inner loop, so that at any moment the whole grid gathers from ONE draw -- a slice
// of N D doubles, which the caches hold, as in a merge of dense rows.  Draws side by side (in grid rows, or several per
// thread in registers) were measured slower per draw, up to 3 times.  Every element of y is read once.
//   image t   sum over the covering patches in increasing n, NaN skipped, divided by the count; none valid: NaN -- the
//             operations of patches_mean_kernel in its order.  Stored when imgs != NULL: imgs (n, H, W, C).
//   moments   Welford over the images in draw order from mean = 0, M2 = 0: delta = x_t - mean, mean += delta / t,
//             M2 += delta (x_t - mean); mean_out = mean, std_out = sqrt(M2 / n) (ddof 0).  A NaN image makes both NaN;
//             identical images give their value and exactly 0 (evo_amd.utils.prepost.image_moments_host is the mirror).
//             Either may be NULL.
__global__ void __launch_bounds__(256) patches_mean_draws_kernel(const double *__restrict__ y, i64 T, int t0, int n, PatchGeom g,
                                                                 double *__restrict__ imgs, double *__restrict__ mean_out,
                                                                 double *__restrict__ std_out) {
#pragma clang fp contract(off)
  const i64 total = (i64)g.H * g.W * g.C;
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % g.C);
  const i64 px = e / g.C;
  const int py = (int)(px / g.W), x = (int)(px - (i64)py * g.W);
  int r0, r1, c0, c1;
  patch_cover(py, g.H, g.ph, g.s, g.nr, r0, r1);
  patch_cover(x, g.W, g.pw, g.s, g.nc, c0, c1);
  double mean = 0.0, M2 = 0.0;
  for (int t = 0; t < n; t++) {
    const PatchDrawRows src{y, T, t0 + t};
    double sum = 0.0;
    int cnt = 0;
    for (int ir = r0; ir <= r1; ir++)
      for (int ic = c0; ic <= c1; ic++) {
        const double v = patch_estimate(src, g, ir, ic, py, x, c);
        if (v == v) {
          sum += v;
          cnt++;
        }
      }
    const double v = cnt ? sum / (double)cnt : __builtin_nan("");
    if (imgs) imgs[(i64)t * total + e] = v;
    const double delta = v - mean;
    mean += delta / (double)(t + 1);
    M2 += delta * (v - mean);
  }
  if (mean_out) mean_out[e] = mean;
  if (std_out) std_out[e] = sqrt(M2 / (double)n);
}

// The same moments over n images (n, total) already on the device (the median merge of draws leaves them there): one
// thread per output element, Welford in draw order as above.
__global__ void __launch_bounds__(256) patches_moments_kernel(const double *__restrict__ imgs, int n, i64 total,
                                                              double *__restrict__ mean_out, double *__restrict__ std_out) {
#pragma clang fp contract(off)
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  double mean = 0.0, M2 = 0.0;
  for (int t = 0; t < n; t++) {
    const double v = imgs[(i64)t * total + e];
    const double delta = v - mean;
    mean += delta / (double)(t + 1);
    M2 += delta * (v - mean);
  }
  if (mean_out) mean_out[e] = mean;
  if (std_out) std_out[e] = sqrt(M2 / (double)n);
}

// Precision-weighted mean merge: out = (sum_k e_k w_k) / (sum_k w_k), w_k = 1 / v_k, over the covering patches in
// increasing n; multiply and add are separate IEEE operations (no contraction), both sums start from 0.0.  An estimate
// that is NaN, or whose variance is NaN or <= 0, is skipped; no valid estimate gives NaN.  One thread per output element,
// like the mean merge; bit-identical to evo_amd.utils.prepost.PrecisionMerger.
__global__ void __launch_bounds__(256) patches_wmean_kernel(PatchRows est, PatchRows var, PatchGeom g, double *__restrict__ out) {
#pragma clang fp contract(off)
  const i64 total = (i64)g.H * g.W * g.C;
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % g.C);
  const i64 px = e / g.C;
  const int y = (int)(px / g.W), x = (int)(px - (i64)y * g.W);
  int r0, r1, c0, c1;
  patch_cover(y, g.H, g.ph, g.s, g.nr, r0, r1);
  patch_cover(x, g.W, g.pw, g.s, g.nc, c0, c1);
  double num = 0.0, den = 0.0;
  int cnt = 0;
  for (int ir = r0; ir <= r1; ir++)
    for (int ic = c0; ic <= c1; ic++) {
      const double v = patch_estimate(est, g, ir, ic, y, x, c);
      const double s = patch_estimate(var, g, ir, ic, y, x, c);
      if (v == v && s > 0.0) {  // (s > 0 is false for NaN)
        const double w = 1.0 / s;
        num += v * w;
        den += w;
        cnt++;
      }
    }
  out[e] = cnt ? num / den : __builtin_nan("");
}

// Median merge: a bitonic sort of every output element's estimates across the lanes of a wave (and, for more than 64
// estimates, across R registers per lane: element index = r * 64 + lane).  R = 1: segments of P lanes (P = the power of
// two >= the largest estimate count, <= 64), 64 / P output elements per wave; R > 1: P = 64 R, one element per wave.
// NaN and the padding sort as +inf; the count of valid estimates picks the middle ones.  Registers: R doubles per lane.
template <int R, class Src>
__global__ void __launch_bounds__(256) patches_median_kernel(Src src, PatchGeom g, int P, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int lane = lane_id();
  const int seg = R == 1 ? P : 64;  // lanes per output element
  const int sl = lane % seg;        // lane within the segment
  const i64 total = (i64)g.H * g.W * g.C;
  const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const i64 e = wave * (64 / seg) + lane / seg;
  const bool live = e < total;
  int y = 0, x = 0, c = 0, r0 = 0, c0 = 0, kc = 1, K = 0;
  if (live) {
    c = (int)(e % g.C);
    const i64 px = e / g.C;
    y = (int)(px / g.W), x = (int)(px - (i64)y * g.W);
    int r1, c1;
    patch_cover(y, g.H, g.ph, g.s, g.nr, r0, r1);
    patch_cover(x, g.W, g.pw, g.s, g.nc, c0, c1);
    kc = c1 - c0 + 1;
    K = (r1 - r0 + 1) * kc;
  }
  const double inf = __builtin_inf();
  double v[R];
  int nvalid = 0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int k = r * 64 + sl;
    double t = inf;
    bool ok = false;
    if (k < K) {
      const int ir = r0 + k / kc, ic = c0 + k % kc;
      t = patch_estimate(src, g, ir, ic, y, x, c);
      ok = t == t;
      if (!ok) t = inf;
    }
    v[r] = t;
    const u64 segmask = seg == 64 ? ~0ull : (((1ull << seg) - 1) << (lane - sl));
    nvalid += __popcll(__ballot(ok) & segmask);
  }
  // bitonic network over P elements
  for (int k2 = 2; k2 <= (R == 1 ? P : 64 * R); k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int jr = j >> 6;
          if (r & jr) continue;
          const bool asc = ((r * 64) & k2) == 0;
          // partner register r | jr, selected without a dynamic register index
#pragma unroll
          for (int r2 = 0; r2 < R; r2++) {
            if (r2 != (r | jr)) continue;
            const double a = v[r], b = v[r2];
            const bool sw = asc ? (b < a) : (a < b);
            v[r] = sw ? b : a;
            v[r2] = sw ? a : b;
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; r++) {
          const double p = __shfl_xor(v[r], j, 64);
          const bool asc = (((r * 64) + sl) & k2) == 0;
          const bool lower = (sl & j) == 0;
          const bool keep_min = asc == lower;
          v[r] = keep_min ? (p < v[r] ? p : v[r]) : (p > v[r] ? p : v[r]);
        }
      }
    }
  }
  // sorted element i lives in register i / 64 of lane (segment base + i % 64)
  const int base = lane - sl;
  const int ilo = nvalid > 0 ? (nvalid - 1) / 2 : 0, ihi = nvalid / 2;
  double tlo = v[0], thi = v[0];
#pragma unroll
  for (int r = 1; r < R; r++) {
    if (r == ilo / 64) tlo = v[r];
    if (r == ihi / 64) thi = v[r];
  }
  const double lo = __shfl(tlo, base + ilo % 64, 64);
  const double hi = __shfl(thi, base + (ihi < (R == 1 ? P : 64 * R) ? ihi : 0) % 64, 64);
  if (live && sl == 0) {
    double m;
    if (nvalid == 0)
      m = __builtin_nan("");
    else if (nvalid & 1)
      m = lo;
    else
      m = (lo + hi) / 2.0;
    out[src.image() * total + e] = m;
  }
}
