// Evaluation metrics on the device (include/him.h "Evaluation metrics"): SSIM / squared / absolute error sums of two
// image batches inside an optional per-sample box, and the integer confusion matrix of a predicted label plane.
//
// him_image_metrics: one 256-thread workgroup owns a tile of MET_TH x MET_TW = 16 x 64 window origins (and, for the
// error sums, the same 16 x 64 pixels).  It stages the (16+10) x (64+10) pixels of BOTH images once in LDS, as
// differences to a per-tile pivot (the tile's first pixel): variance and covariance do not move under a shift, and the
// moments of the small differences do not cancel the way E[x^2] - mu^2 does on a bright flat region.  The row pass
// writes the five horizontal moments to LDS, the column pass reads them back (lane = column in both passes: consecutive
// dwords, no bank conflict) and evaluates the formula.  Each workgroup writes three doubles to its own workspace slot;
// a second launch adds the slots of a plane in a fixed order.  No floating-point atomics anywhere.
//
// him_confusion: each workgroup counts its share of pixels into a private 32-bit LDS histogram while n <= CONF_LDS_MAX_N
// (n * n * 4 bytes <= 100 KiB of the CU's 160 KiB) and flushes the non-zero cells with 64-bit integer atomics; above
// that it adds to the int64 matrix directly.  A wave whose 64 pixels fall into one cell adds 64 once.
#include <math.h>

#include "him_common.h"

namespace him {

#define MET_WIN 11
#define MET_HALO (MET_WIN - 1)
#define MET_TH 16
#define MET_TW 64
#define MET_SH (MET_TH + MET_HALO)  // staged rows
#define MET_SW (MET_TW + MET_HALO)  // staged columns
#define MET_PART 3                  // doubles per workgroup: ssim sum, squared error sum, absolute error sum

struct MetGauss {
  float g[MET_WIN];
};

struct MetParams {
  float scale, offset, c1, c2;
  int quantize, preset;  // preset: the tensor2im operation order (x + 1) / 2 * 255
};

// x' = x * scale + offset, both rounded to fp32 on their own; the (127.5, 127.5, quantize) preset takes tensor2im's
// order (x + 1) / 2 * 255 so that the value is the byte him_tensor2im_bytes(normalize = 1) writes
__device__ __forceinline__ float met_map(float x, const MetParams& p) {
  float v = p.preset ? __fmul_rn(__fmul_rn(__fadd_rn(x, 1.0f), 0.5f), 255.0f) : __fadd_rn(__fmul_rn(x, p.scale), p.offset);
  if (p.quantize) v = truncf(fminf(fmaxf(v, 0.0f), 255.0f));
  return v;
}

// the clipped box of sample b: origin (x0, y0), size (w, h); h <= 0 or w <= 0: empty
__device__ __forceinline__ void met_region(const int* __restrict__ box, int b, int H, int W, int& x0, int& y0, int& w, int& h) {
  if (box == nullptr) {
    x0 = 0, y0 = 0, w = W, h = H;
    return;
  }
  const int xa = max(box[4 * b + 0], 0), ya = max(box[4 * b + 1], 0);
  const int xb = min(box[4 * b + 2], W - 1), yb = min(box[4 * b + 3], H - 1);
  x0 = xa, y0 = ya;
  w = xb >= xa ? xb - xa + 1 : 0;
  h = yb >= ya ? yb - ya + 1 : 0;
}

__global__ __launch_bounds__(256) void image_metrics_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const int* __restrict__ box, int C, int H, int W,
                                                                 MetParams prm, MetGauss gw, double* __restrict__ part,
                                                                 float* __restrict__ map_out) {
  __shared__ float sa[MET_SH][MET_SW], sb[MET_SH][MET_SW];
  __shared__ float mom[5][MET_SH][MET_TW];
  __shared__ double red[3][4];
  const int plane = blockIdx.z, tid = threadIdx.x;
  const int tiles_x = gridDim.x;
  double* slot = part + ((size_t)plane * gridDim.y * tiles_x + (size_t)blockIdx.y * tiles_x + blockIdx.x) * MET_PART;
  int x0, y0, w, h;
  met_region(box, plane / C, H, W, x0, y0, w, h);
  const int ty0 = blockIdx.y * MET_TH, tx0 = blockIdx.x * MET_TW;  // tile origin inside the region
  if (h <= 0 || w <= 0 || ty0 >= h || tx0 >= w) {                   // uniform for the workgroup
    if (tid < MET_PART) slot[tid] = 0.0;
    return;
  }
  const float* pa = a + (size_t)plane * H * W + (size_t)y0 * W + x0;
  const float* pb = b + (size_t)plane * H * W + (size_t)y0 * W + x0;
  const float piv_a = met_map(pa[(size_t)ty0 * W + tx0], prm), piv_b = met_map(pb[(size_t)ty0 * W + tx0], prm);

  // stage both images (differences to the pivots); the pixels this tile owns feed the error sums as they pass
  double sq = 0.0, ab = 0.0;
  for (int i = tid; i < MET_SH * MET_SW; i += 256) {
    const int r = i / MET_SW, c = i - r * MET_SW;
    const int y = ty0 + r, x = tx0 + c;
    float da = 0.0f, db = 0.0f;
    if (y < h && x < w) {
      const float va = met_map(pa[(size_t)y * W + x], prm), vb = met_map(pb[(size_t)y * W + x], prm);
      da = __fsub_rn(va, piv_a);
      db = __fsub_rn(vb, piv_b);
      if (r < MET_TH && c < MET_TW) {
        const double d = (double)va - (double)vb;
        sq += d * d;
        ab += fabs(d);
      }
    }
    sa[r][c] = da;
    sb[r][c] = db;
  }
  __syncthreads();

  const int col = tid & 63, rg = tid >> 6;
  // row pass: the five horizontal moments of every staged row at this thread's column
  for (int r = rg; r < MET_SH; r += 4) {
    float ma = 0.0f, mb = 0.0f, maa = 0.0f, mbb = 0.0f, mab = 0.0f;
#pragma unroll
    for (int k = 0; k < MET_WIN; ++k) {
      const float va = sa[r][col + k], vb = sb[r][col + k], g = gw.g[k];
      ma = fmaf(g, va, ma);
      mb = fmaf(g, vb, mb);
      maa = fmaf(g, __fmul_rn(va, va), maa);
      mbb = fmaf(g, __fmul_rn(vb, vb), mbb);
      mab = fmaf(g, __fmul_rn(va, vb), mab);
    }
    mom[0][r][col] = ma;
    mom[1][r][col] = mb;
    mom[2][r][col] = maa;
    mom[3][r][col] = mbb;
    mom[4][r][col] = mab;
  }
  __syncthreads();

  // column pass: this thread's column, output rows 4 rg .. 4 rg + 3
  constexpr int RPT = MET_TH / 4;
  float e[5][RPT];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float v[RPT + MET_HALO];
#pragma unroll
    for (int j = 0; j < RPT + MET_HALO; ++j) v[j] = mom[q][rg * RPT + j][col];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < MET_WIN; ++k) s = fmaf(gw.g[k], v[j + k], s);
      e[q][j] = s;
    }
  }
  const int mh = h - MET_HALO, mw = w - MET_HALO;  // the window map of the region
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int oy = ty0 + rg * RPT + j, ox = tx0 + col;
    if (oy < mh && ox < mw) {
      const float ea = e[0][j], eb = e[1][j];
      const float mua = __fadd_rn(piv_a, ea), mub = __fadd_rn(piv_b, eb);
      const float va = __fsub_rn(e[2][j], __fmul_rn(ea, ea)), vb = __fsub_rn(e[3][j], __fmul_rn(eb, eb));
      const float cab = __fsub_rn(e[4][j], __fmul_rn(ea, eb));
      const float num = __fmul_rn(__fadd_rn(__fmul_rn(__fmul_rn(2.0f, mua), mub), prm.c1),
                                  __fadd_rn(__fmul_rn(2.0f, cab), prm.c2));
      const float den = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(mua, mua), __fmul_rn(mub, mub)), prm.c1),
                                  __fadd_rn(__fadd_rn(va, vb), prm.c2));
      const float s = __fdiv_rn(num, den);
      ss += (double)s;
      if (map_out != nullptr) map_out[((size_t)plane * (H - MET_HALO) + oy) * (W - MET_HALO) + ox] = s;
    }
  }
  ss = wave_sum_f64(ss);
  sq = wave_sum_f64(sq);
  ab = wave_sum_f64(ab);
  if (col == 0) red[0][rg] = ss, red[1][rg] = sq, red[2][rg] = ab;
  __syncthreads();
  if (tid < MET_PART) slot[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// one workgroup per plane: thread t adds the slots t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void image_metrics_sum_kernel(const double* __restrict__ part, int tiles,
                                                                const int* __restrict__ box, int C, int H, int W,
                                                                double* __restrict__ sums) {
  __shared__ double red[MET_PART][256];
  const int plane = blockIdx.x, tid = threadIdx.x;
  double acc[MET_PART] = {0.0, 0.0, 0.0};
  for (int t = tid; t < tiles; t += 256)
#pragma unroll
    for (int q = 0; q < MET_PART; ++q) acc[q] += part[((size_t)plane * tiles + t) * MET_PART + q];
#pragma unroll
  for (int q = 0; q < MET_PART; ++q) red[q][tid] = acc[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int q = 0; q < MET_PART; ++q) red[q][tid] += red[q][tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    int x0, y0, w, h;
    met_region(box, plane / C, H, W, x0, y0, w, h);
    const bool empty = h <= 0 || w <= 0;
    double* o = sums + (size_t)plane * 5;
    o[0] = red[0][0];
    o[1] = empty ? 0.0 : (double)max(h - MET_HALO, 0) * (double)max(w - MET_HALO, 0);
    o[2] = red[1][0];
    o[3] = red[2][0];
    o[4] = empty ? 0.0 : (double)h * (double)w;
  }
}

static inline int met_tiles_x(int W) { return (W + MET_TW - 1) / MET_TW; }
static inline int met_tiles_y(int H) { return (H + MET_TH - 1) / MET_TH; }
static inline size_t met_ws_bytes(int B, int C, int H, int W) {
  return (size_t)B * C * met_tiles_x(W) * met_tiles_y(H) * MET_PART * sizeof(double);
}

// ---------------------------------------------------------------------------------------------------- confusion matrix
#define CONF_LDS_MAX_N 160  // private LDS histogram up to 160 x 160 32-bit counters (100 KiB)
#define CONF_PX 4           // pixels per thread and step (the vector width of the aligned path)
#define CONF_WS_BYTES 16    // one 64-bit count of skipped pixels (+ padding)

#define CONF_INVALID (-1)
#define CONF_IGNORED (-2)

__device__ __forceinline__ int conf_id(unsigned char v, int n) { return (int)v < n ? (int)v : CONF_INVALID; }
__device__ __forceinline__ int conf_id(int v, int n) { return (v >= 0 && v < n) ? v : CONF_INVALID; }
__device__ __forceinline__ int conf_id(long long v, int n) { return (v >= 0 && v < (long long)n) ? (int)v : CONF_INVALID; }
__device__ __forceinline__ int conf_id(float v, int n) {
  return (v >= 0.0f && v < (float)n && v == floorf(v)) ? (int)v : CONF_INVALID;
}
__device__ __forceinline__ bool conf_is(unsigned char v, int id) { return (int)v == id; }
__device__ __forceinline__ bool conf_is(int v, int id) { return v == id; }
__device__ __forceinline__ bool conf_is(long long v, int id) { return v == (long long)id; }
__device__ __forceinline__ bool conf_is(float v, int id) { return v == (float)id; }

template <typename T>
__device__ __forceinline__ void conf_load(const T* __restrict__ plane, long long i0, long long n, bool vec, T v[CONF_PX]) {
  if (vec) {
    struct alignas(sizeof(T) * CONF_PX < 16 ? sizeof(T) * CONF_PX : 16) Q { T a[CONF_PX]; };
    const Q q = *(const Q*)(plane + i0);
#pragma unroll
    for (int k = 0; k < CONF_PX; ++k) v[k] = q.a[k];
  } else {
#pragma unroll
    for (int k = 0; k < CONF_PX; ++k) v[k] = i0 + k < n ? plane[i0 + k] : T(0);
  }
}

__global__ void conf_clear_kernel(long long* __restrict__ counts, long long cells, unsigned long long* __restrict__ ws) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < cells; i += (long long)gridDim.x * blockDim.x)
    counts[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) ws[0] = 0ull;
}

__global__ void conf_status_kernel(const unsigned long long* __restrict__ ws, int accumulate, int* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned long long s = ws[0];
  int flags = s ? HIM_CONF_SKIPPED : 0;
  if (accumulate) {
    s += (unsigned long long)(unsigned)max(status[0], 0);
    flags |= status[1];
  }
  if (s > 0x7fffffffull) s = 0x7fffffffull, flags |= HIM_CONF_SATURATED;
  status[0] = (int)s;
  status[1] = flags;
}

// PK: 0 ids of type TP, 4 scores (TP = float, C channels), 5 probabilities (TP = float).  Workgroup (x, b) owns the
// groups [x * per, (x + 1) * per) of CONF_PX pixels of sample b.  LDS = true: private histogram of n * n counters.
template <typename TP, typename TG, int PK, bool LDS>
__global__ __launch_bounds__(256) void confusion_kernel(const TP* __restrict__ pred, const TG* __restrict__ gt,
                                                        const float* __restrict__ mask, int C, long long hw, int vec,
                                                        int n, int ignore, int per_sample, long long per,
                                                        unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned conf_hist[];
  __shared__ unsigned conf_skipped;
  const int tid = threadIdx.x, b = blockIdx.y, cells = n * n;
  if (LDS)
    for (int i = tid; i < cells; i += 256) conf_hist[i] = 0u;
  if (tid == 0) conf_skipped = 0u;
  __syncthreads();
  const TP* pp = pred + (size_t)b * (PK == 4 ? C : 1) * hw;
  const TG* pg = gt + (size_t)b * hw;
  const float* pm = mask ? mask + (size_t)b * hw : nullptr;
  unsigned long long* out = counts + (per_sample ? (size_t)b * cells : 0);
  const long long groups = (hw + CONF_PX - 1) / CONF_PX;
  const long long g0 = blockIdx.x * per, g1 = min(g0 + per, groups);
  unsigned skipped = 0;
  // the trip count is uniform for the workgroup: every lane reaches the whole-wave test below
  for (long long gb = g0; gb < g1; gb += 256) {
    const long long g = gb + tid;
    int cell[CONF_PX];
#pragma unroll
    for (int k = 0; k < CONF_PX; ++k) cell[k] = -1;
    if (g < g1) {
      const long long i0 = g * CONF_PX;
      TG vg[CONF_PX];
      float vm[CONF_PX];
      int lab[CONF_PX];
      conf_load(pg, i0, hw, vec != 0, vg);
      if (pm) conf_load(pm, i0, hw, vec != 0, vm);
      if (PK == 4) {
        float best[CONF_PX];
        conf_load((const float*)pp, i0, hw, vec != 0, best);
#pragma unroll
        for (int k = 0; k < CONF_PX; ++k) lab[k] = 0;
        for (int c = 1; c < C; ++c) {  // strict > walking upwards: the lowest channel of the maximum
          float v[CONF_PX];
          conf_load((const float*)pp + (size_t)c * hw, i0, hw, vec != 0, v);
#pragma unroll
          for (int k = 0; k < CONF_PX; ++k)
            if (v[k] > best[k]) best[k] = v[k], lab[k] = c;
        }
#pragma unroll
        for (int k = 0; k < CONF_PX; ++k) lab[k] = lab[k] < n ? lab[k] : CONF_INVALID;
      } else {
        TP vp[CONF_PX];
        conf_load(pp, i0, hw, vec != 0, vp);
#pragma unroll
        for (int k = 0; k < CONF_PX; ++k) {
          if (PK == 5) {
            const int l = (float)vp[k] > 0.5f ? 1 : 0;
            lab[k] = l < n ? l : CONF_INVALID;
          } else {
            lab[k] = conf_id(vp[k], n);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < CONF_PX; ++k) {
        if (i0 + k >= hw) continue;
        if (pm && vm[k] == 0.0f) continue;
        if (ignore >= 0 && conf_is(vg[k], ignore)) continue;
        const int row = conf_id(vg[k], n);
        if (row < 0 || lab[k] < 0) {
          ++skipped;
          continue;
        }
        cell[k] = row * n + lab[k];
      }
    }
#pragma unroll
    for (int k = 0; k < CONF_PX; ++k) {
      const int first = __builtin_amdgcn_readfirstlane(cell[k]);
      if (__all(cell[k] == first)) {  // the whole wave in one cell (or nothing to count): one add of 64
        if (first >= 0 && (tid & 63) == 0) {
          if (LDS) atomicAdd(&conf_hist[first], 64u);
          else atomicAdd(&out[first], 64ull);
        }
      } else if (cell[k] >= 0) {
        if (LDS) atomicAdd(&conf_hist[cell[k]], 1u);
        else atomicAdd(&out[cell[k]], 1ull);
      }
    }
  }
  if (skipped) atomicAdd(&conf_skipped, skipped);
  __syncthreads();
  if (LDS)
    for (int i = tid; i < cells; i += 256) {
      const unsigned v = conf_hist[i];
      if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
  if (tid == 0 && conf_skipped) atomicAdd(&ws[0], (unsigned long long)conf_skipped);
}

template <typename TP, typename TG, int PK>
static void conf_launch2(const void* pred, const void* gt, const float* mask, int B, int C, long long hw, int vec, int n,
                         int ignore, int per_sample, unsigned long long* counts, unsigned long long* ws, hipStream_t st) {
  const long long groups = (hw + CONF_PX - 1) / CONF_PX;
  const bool lds = n <= CONF_LDS_MAX_N;
  // at least 512 groups (2 048 pixels) per workgroup; fewer, larger shares when the private histogram is large to flush
  const long long cap = (lds && n <= 64 ? 4LL : 1LL) * device_cus();
  long long wgs = (groups + 511) / 512;
  wgs = wgs < 1 ? 1 : wgs;
  const long long per_b = cap / B > 0 ? cap / B : 1;
  if (wgs > per_b) wgs = per_b;
  long long per = (groups + wgs - 1) / wgs;
  per = (per + 255) / 256 * 256;               // whole 256-group steps: the shares do not overlap inside a step
  wgs = (groups + per - 1) / per;              // per * CONF_PX pixels per workgroup, < 2^32 as hw <= 2^31 - 1
  const dim3 grid((unsigned)wgs, (unsigned)B);
  if (lds) {
    const size_t bytes = (size_t)n * n * sizeof(unsigned);
    (void)hipFuncSetAttribute((const void*)confusion_kernel<TP, TG, PK, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              CONF_LDS_MAX_N * CONF_LDS_MAX_N * (int)sizeof(unsigned));
    hipLaunchKernelGGL((confusion_kernel<TP, TG, PK, true>), grid, dim3(256), bytes, st, (const TP*)pred, (const TG*)gt,
                       mask, C, hw, vec, n, ignore, per_sample, per, counts, ws);
  } else {
    hipLaunchKernelGGL((confusion_kernel<TP, TG, PK, false>), grid, dim3(256), 0, st, (const TP*)pred, (const TG*)gt, mask,
                       C, hw, vec, n, ignore, per_sample, per, counts, ws);
  }
}

template <typename TG>
static void conf_launch1(const void* pred, int pred_kind, const void* gt, const float* mask, int B, int C, long long hw,
                         int vec, int n, int ignore, int per_sample, unsigned long long* counts, unsigned long long* ws,
                         hipStream_t st) {
#define CONF_GO(TP, PK) conf_launch2<TP, TG, PK>(pred, gt, mask, B, C, hw, vec, n, ignore, per_sample, counts, ws, st)
  switch (pred_kind) {
    case 0: CONF_GO(unsigned char, 0); break;
    case 1: CONF_GO(int, 0); break;
    case 2: CONF_GO(long long, 0); break;
    case 3: CONF_GO(float, 0); break;
    case 4: CONF_GO(float, 4); break;
    default: CONF_GO(float, 5); break;
  }
#undef CONF_GO
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_image_metrics_workspace(int B, int C, int H, int W) {
  if (B <= 0 || (C != 1 && C != 3) || H <= 0 || W <= 0) return 0;
  return met_ws_bytes(B, C, H, W);
}

int him_image_metrics(const float* a, const float* b, int B, int C, int H, int W, float scale, float offset, int quantize,
                      float data_range, const int* box, double* sums, float* map_out, void* ws, size_t ws_bytes,
                      void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
    return fail(HIM_E_INVALID, "image_metrics: bad shape");
  if (C != 1 && C != 3) return fail(HIM_E_INVALID, "image_metrics: %d channels (1 or 3)", C);
  if ((long long)B * C > 65535) return fail(HIM_E_INVALID, "image_metrics: %d planes (at most 65535)", B * C);
  if (met_tiles_y(H) > 65535) return fail(HIM_E_INVALID, "image_metrics: %d rows (at most %d)", H, 65535 * MET_TH);
  if (!a || !b || !sums || !ws) return fail(HIM_E_INVALID, "image_metrics: null pointer");
  if (!(data_range > 0.0f)) return fail(HIM_E_INVALID, "image_metrics: data_range must be positive");
  if (map_out && box) return fail(HIM_E_INVALID, "image_metrics: map_out is written for whole-image calls only");
  if (map_out && (H < MET_WIN || W < MET_WIN)) return fail(HIM_E_INVALID, "image_metrics: map_out of an image below 11x11");
  if ((uintptr_t)ws % 8 != 0 || (uintptr_t)sums % 8 != 0)
    return fail(HIM_E_INVALID, "image_metrics: sums / workspace not 8-byte aligned");
  if ((uintptr_t)a % 4 != 0 || (uintptr_t)b % 4 != 0) return fail(HIM_E_INVALID, "image_metrics: image not 4-byte aligned");
  const size_t need = met_ws_bytes(B, C, H, W);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "image_metrics: workspace %zu < %zu bytes", ws_bytes, need);
  MetGauss gw;
  double g[MET_WIN], total = 0.0;
  for (int i = 0; i < MET_WIN; ++i) total += g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
  for (int i = 0; i < MET_WIN; ++i) gw.g[i] = (float)(g[i] / total);
  MetParams prm;
  prm.scale = scale, prm.offset = offset, prm.quantize = quantize ? 1 : 0;
  prm.preset = (quantize && scale == 127.5f && offset == 127.5f) ? 1 : 0;
  const double k1 = 0.01 * (double)data_range, k2 = 0.03 * (double)data_range;
  prm.c1 = (float)(k1 * k1), prm.c2 = (float)(k2 * k2);
  const int tx = met_tiles_x(W), ty = met_tiles_y(H);
  hipLaunchKernelGGL(image_metrics_tile_kernel, dim3(tx, ty, B * C), dim3(256), 0, ST, a, b, box, C, H, W, prm, gw,
                     (double*)ws, map_out);
  hipLaunchKernelGGL(image_metrics_sum_kernel, dim3(B * C), dim3(256), 0, ST, (const double*)ws, tx * ty, box, C, H, W, sums);
  return check_launch("image_metrics");
}

size_t him_confusion_workspace(int n) { return (n >= 1 && n <= 256) ? CONF_WS_BYTES : 0; }

int him_confusion(const void* pred, int pred_kind, const void* gt, int gt_kind, const float* mask, int B, int C, int H,
                  int W, int n, int ignore, int per_sample, int accumulate, long long* counts, int* status, void* ws,
                  size_t ws_bytes, void* stream) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
    return fail(HIM_E_INVALID, "confusion: bad shape");
  if (n < 1 || n > 256) return fail(HIM_E_INVALID, "confusion: n %d (1..256)", n);
  if (pred_kind < 0 || pred_kind > 5) return fail(HIM_E_INVALID, "confusion: pred_kind %d", pred_kind);
  if (gt_kind < 0 || gt_kind > 3) return fail(HIM_E_INVALID, "confusion: gt_kind %d", gt_kind);
  if (pred_kind == 4 ? C < 1 : C != 1) return fail(HIM_E_INVALID, "confusion: C %d for pred_kind %d", C, pred_kind);
  if (ignore < -1) return fail(HIM_E_INVALID, "confusion: ignore %d (-1 or an id)", ignore);
  if (!pred || !gt || !counts || !status || !ws) return fail(HIM_E_INVALID, "confusion: null pointer");
  if ((uintptr_t)counts % 8 != 0 || (uintptr_t)ws % 8 != 0 || (uintptr_t)status % 4 != 0)
    return fail(HIM_E_INVALID, "confusion: counts / workspace / status misaligned");
  static const int esize[6] = {1, 4, 8, 4, 4, 4};
  if ((uintptr_t)pred % esize[pred_kind] != 0 || (uintptr_t)gt % esize[gt_kind] != 0 || (uintptr_t)mask % 4 != 0)
    return fail(HIM_E_INVALID, "confusion: plane not aligned to its element size");
  if (ws_bytes < CONF_WS_BYTES) return fail(HIM_E_WORKSPACE, "confusion: workspace %zu < %d bytes", ws_bytes, CONF_WS_BYTES);
  const long long hw = (long long)H * W;
  const int vec = (W % CONF_PX == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)gt % 16 == 0 && (uintptr_t)mask % 16 == 0) ? 1 : 0;
  const long long cells = accumulate ? 0 : (long long)(per_sample ? B : 1) * n * n;
  unsigned long long* cnt = (unsigned long long*)counts;
  unsigned long long* w = (unsigned long long*)ws;
  hipLaunchKernelGGL(conf_clear_kernel, dim3(cells > 65536 ? 256 : (cells > 256 ? (unsigned)((cells + 255) / 256) : 1)),
                     dim3(256), 0, ST, counts, cells, w);
  switch (gt_kind) {
    case 0: conf_launch1<unsigned char>(pred, pred_kind, gt, mask, B, C, hw, vec, n, ignore, per_sample ? 1 : 0, cnt, w, ST); break;
    case 1: conf_launch1<int>(pred, pred_kind, gt, mask, B, C, hw, vec, n, ignore, per_sample ? 1 : 0, cnt, w, ST); break;
    case 2: conf_launch1<long long>(pred, pred_kind, gt, mask, B, C, hw, vec, n, ignore, per_sample ? 1 : 0, cnt, w, ST); break;
    default: conf_launch1<float>(pred, pred_kind, gt, mask, B, C, hw, vec, n, ignore, per_sample ? 1 : 0, cnt, w, ST); break;
  }
  hipLaunchKernelGGL(conf_status_kernel, dim3(1), dim3(64), 0, ST, (const unsigned long long*)w, accumulate ? 1 : 0, status);
  return check_launch("confusion");
}

}  // extern "C"
