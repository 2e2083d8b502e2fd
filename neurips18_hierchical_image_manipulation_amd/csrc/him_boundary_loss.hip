// Boundary-weighted and surface losses of the box2mask trainer (include/him.h "Boundary-weighted and surface losses").
// The weight of a pixel is a function of its int32 squared distance (a him_edt plane): forward and backward read the
// distance planes and recompute it, no weight plane ever exists in memory.  HBM-bound streams; sums by a two-stage
// fixed-order reduction in double (no atomics, bit-identical from run to run).
#include <algorithm>
#include <cmath>

#include "him_common.h"

namespace him {

static const int BW_BLOCKS = 64;      // fixed forward grid: one double pair per workgroup, added by one workgroup in slot order
static const int BW_BWD_BLOCKS = 2048;

#define BW_LOOP(i, n) \
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)(n); i += (long long)gridDim.x * 256)

// w = 1 + amp * exp(-d2 / den), den = 2 sigma^2; exactly 1 without a boundary in the plane, exactly 1 + amp on one
__device__ __forceinline__ float bw_weight(int d2, float amp, float den) {
  if (d2 == HIM_EDT_NONE) return 1.f;
  return 1.f + amp * (d2 == 0 ? 1.f : expf(-(float)d2 / den));
}

__device__ __forceinline__ float pair_term(float p, float t, int kind) {
  if (kind == 1) return fabsf(p - t);
  return -(t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(logf(1.f - p), -100.f));
}

// signed distance to the mask's outline: positive outside (to the nearest t == 1), negative inside (to the nearest t == 0)
__device__ __forceinline__ float surface_phi(float t, int d2_fg, int d2_bg) {
  if (t < 0.5f) return d2_fg == HIM_EDT_NONE ? 0.f : sqrtf((float)d2_fg);
  return d2_bg == HIM_EDT_NONE ? 0.f : -sqrtf((float)d2_bg);
}

// slot[blockIdx.x * 2 + {0,1}] = the workgroup's two sums
__device__ __forceinline__ void bw_store_pair(float a, float b, double* __restrict__ slot, double* sh) {
  const double da = block_sum_f64((double)a, sh);
  const double db = block_sum_f64((double)b, sh);
  if (threadIdx.x == 0) {
    slot[blockIdx.x * 2] = da;
    slot[blockIdx.x * 2 + 1] = db;
  }
}

__global__ __launch_bounds__(256) void bw_nll_stage1(const float* __restrict__ logp, const float* __restrict__ label,
                                                     const float* __restrict__ mask, const int* __restrict__ dist2,
                                                     double* __restrict__ slot, int B, int C, int hw, float amp, float den) {
  __shared__ double sh[4];
  const long long n = (long long)B * hw;
  float a = 0.f, sw = 0.f;
  BW_LOOP(i, n) {
    const int b = (int)(i / hw), r = (int)(i - (long long)b * hw);
    const int id = (int)label[i];
    if (mask[i] >= 0.5f && id >= 0 && id < C) {
      const float w = bw_weight(dist2[i], amp, den);
      a -= w * logp[((size_t)b * C + id) * hw + r];
      sw += w;
    }
  }
  bw_store_pair(a, sw, slot, sh);
}

__global__ __launch_bounds__(256) void bw_pair_stage1(const float* __restrict__ p, const float* __restrict__ t,
                                                      const int* __restrict__ dist2, double* __restrict__ slot, long long n,
                                                      int kind, float amp, float den) {
  __shared__ double sh[4];
  float a = 0.f, sw = 0.f;
  BW_LOOP(i, n) {
    const float w = bw_weight(dist2[i], amp, den);
    a += w * pair_term(p[i], t[i], kind);
    sw += w;
  }
  bw_store_pair(a, sw, slot, sh);
}

__global__ __launch_bounds__(256) void surface_stage1(const float* __restrict__ p, const float* __restrict__ t,
                                                      const int* __restrict__ d2_fg, const int* __restrict__ d2_bg,
                                                      double* __restrict__ slot, long long n) {
  __shared__ double sh[4];
  float a = 0.f;
  BW_LOOP(i, n) a += surface_phi(t[i], d2_fg[i], d2_bg[i]) * p[i];
  bw_store_pair(a, 0.f, slot, sh);
}

// one workgroup adds the nb <= BW_BLOCKS slot pairs in a fixed order.  ratio: out2 = {a / s, s} (0/0 = nan when nothing
// is valid, as torch); otherwise out2[0] = a * scale.
__global__ __launch_bounds__(256) void bw_stage2(const double* __restrict__ slot, int nb, int ratio, double scale,
                                                 float* __restrict__ out2) {
  __shared__ double sh[4];
  double a = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    a += slot[i * 2];
    s += slot[i * 2 + 1];
  }
  a = block_sum_f64(a, sh);
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) {
    if (ratio) {
      out2[0] = (float)(a / s);
      out2[1] = (float)s;
    } else {
      out2[0] = (float)(a * scale);
    }
  }
}

// dlogp[b][c][r] = -g * w / sum_w at c = label for valid positions, 0 elsewhere
__global__ __launch_bounds__(256) void bw_nll_bwd_kernel(const float* __restrict__ label, const float* __restrict__ mask,
                                                         const int* __restrict__ dist2, const float* __restrict__ g,
                                                         const float* __restrict__ sum_w, float* __restrict__ dlogp, int B,
                                                         int C, int hw, float amp, float den) {
  const long long n = (long long)B * C * hw;
  const float scale = -g[0] / sum_w[0];
  BW_LOOP(i, n) {
    const int r = (int)(i % hw), c = (int)((i / hw) % C), b = (int)(i / ((long long)hw * C));
    const size_t pi = (size_t)b * hw + r;
    const int id = (int)label[pi];
    dlogp[i] = (mask[pi] >= 0.5f && id == c) ? scale * bw_weight(dist2[pi], amp, den) : 0.f;
  }
}

// the unweighted kernels' derivatives (bce_bwd_kernel, l1_bwd_kernel) times g * w / sum_w
__global__ __launch_bounds__(256) void bw_pair_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                          const int* __restrict__ dist2, const float* __restrict__ g,
                                                          const float* __restrict__ sum_w, float* __restrict__ dp,
                                                          long long n, int kind, float amp, float den) {
  const float scale = g[0] / sum_w[0];
  BW_LOOP(i, n) {
    const float pp = p[i], tt = t[i];
    const float s = scale * bw_weight(dist2[i], amp, den);
    if (kind == 1) {
      const float d = pp - tt;
      dp[i] = d > 0.f ? s : (d < 0.f ? -s : 0.f);
    } else {
      dp[i] = s * (pp - tt) / fmaxf(pp * (1.f - pp), 1e-12f);
    }
  }
}

__global__ __launch_bounds__(256) void surface_bwd_kernel(const float* __restrict__ t, const int* __restrict__ d2_fg,
                                                          const int* __restrict__ d2_bg, const float* __restrict__ g,
                                                          float* __restrict__ dp, long long n, float scale) {
  const float gs = g[0] * scale;
  BW_LOOP(i, n) dp[i] = gs * surface_phi(t[i], d2_fg[i], d2_bg[i]);
}

static inline bool bw_bad_shape(float amp, float sigma) {
  return !std::isfinite(amp) || !std::isfinite(sigma) || amp < 0.f || !(sigma > 0.f);
}
static inline float bw_den(float sigma) { return (float)(2.0 * (double)sigma * (double)sigma); }
static inline int bw_fwd_blocks(long long n) { return (int)std::min<long long>((n + 255) / 256, BW_BLOCKS); }
static inline int bw_bwd_blocks(long long n) { return (int)std::min<long long>((n + 255) / 256, BW_BWD_BLOCKS); }
// 1 / (B*H*W * sqrt(H^2 + W^2)): the image diagonal makes the term a fraction of the plane, whatever its size
static inline double surface_scale(int B, int H, int W) {
  return 1.0 / ((double)B * H * W * std::sqrt((double)H * H + (double)W * W));
}

}  // namespace him

using namespace him;

#define ST ((hipStream_t)stream)

extern "C" {

size_t him_bw_loss_ws(void) { return (size_t)BW_BLOCKS * 2 * sizeof(double) + 256; }

static int bw_ws_check(const char* what, const void* ws, size_t ws_bytes) {
  if (!ws || ws_bytes < him_bw_loss_ws()) return fail(HIM_E_WORKSPACE, "%s: ws too small", what);
  if ((uintptr_t)ws & 7) return fail(HIM_E_INVALID, "%s: ws is not 8-byte aligned", what);
  return HIM_OK;
}

int him_bw_nll_fwd(const float* logp, const float* label, const float* mask, const int* dist2, int B, int C, int hw,
                   float amp, float sigma, float* out2, void* ws, size_t ws_bytes, void* stream) {
  if (!logp || !label || !mask || !dist2 || !out2) return fail(HIM_E_INVALID, "bw_nll: null argument");
  if (B < 1 || C < 1 || hw < 1) return fail(HIM_E_INVALID, "bw_nll: B=%d C=%d hw=%d", B, C, hw);
  if (bw_bad_shape(amp, sigma)) return fail(HIM_E_INVALID, "bw_nll: amp=%g sigma=%g", (double)amp, (double)sigma);
  if (int rc = bw_ws_check("bw_nll", ws, ws_bytes)) return rc;
  const int nb = bw_fwd_blocks((long long)B * hw);
  hipLaunchKernelGGL(bw_nll_stage1, dim3(nb), dim3(256), 0, ST, logp, label, mask, dist2, (double*)ws, B, C, hw, amp,
                     bw_den(sigma));
  hipLaunchKernelGGL(bw_stage2, dim3(1), dim3(256), 0, ST, (const double*)ws, nb, 1, 0.0, out2);
  return check_launch("bw_nll_fwd");
}

int him_bw_nll_bwd(const float* label, const float* mask, const int* dist2, const float* g, const float* sum_w, float amp,
                   float sigma, float* dlogp, int B, int C, int hw, void* stream) {
  if (!label || !mask || !dist2 || !g || !sum_w || !dlogp) return fail(HIM_E_INVALID, "bw_nll_bwd: null argument");
  if (B < 1 || C < 1 || hw < 1) return fail(HIM_E_INVALID, "bw_nll_bwd: B=%d C=%d hw=%d", B, C, hw);
  if (bw_bad_shape(amp, sigma)) return fail(HIM_E_INVALID, "bw_nll_bwd: amp=%g sigma=%g", (double)amp, (double)sigma);
  hipLaunchKernelGGL(bw_nll_bwd_kernel, dim3(bw_bwd_blocks((long long)B * C * hw)), dim3(256), 0, ST, label, mask, dist2, g,
                     sum_w, dlogp, B, C, hw, amp, bw_den(sigma));
  return check_launch("bw_nll_bwd");
}

int him_bw_pair_fwd(const float* p, const float* t, const int* dist2, size_t n, int kind, float amp, float sigma,
                    float* out2, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !t || !dist2 || !out2) return fail(HIM_E_INVALID, "bw_pair: null argument");
  if (n < 1 || n > ((size_t)1 << 40)) return fail(HIM_E_INVALID, "bw_pair: n=%zu", n);
  if (kind != 0 && kind != 1) return fail(HIM_E_INVALID, "bw_pair: kind %d (0 bce, 1 l1)", kind);
  if (bw_bad_shape(amp, sigma)) return fail(HIM_E_INVALID, "bw_pair: amp=%g sigma=%g", (double)amp, (double)sigma);
  if (int rc = bw_ws_check("bw_pair", ws, ws_bytes)) return rc;
  const int nb = bw_fwd_blocks((long long)n);
  hipLaunchKernelGGL(bw_pair_stage1, dim3(nb), dim3(256), 0, ST, p, t, dist2, (double*)ws, (long long)n, kind, amp,
                     bw_den(sigma));
  hipLaunchKernelGGL(bw_stage2, dim3(1), dim3(256), 0, ST, (const double*)ws, nb, 1, 0.0, out2);
  return check_launch("bw_pair_fwd");
}

int him_bw_pair_bwd(const float* p, const float* t, const int* dist2, size_t n, int kind, const float* g,
                    const float* sum_w, float amp, float sigma, float* dp, void* stream) {
  if (!p || !t || !dist2 || !g || !sum_w || !dp) return fail(HIM_E_INVALID, "bw_pair_bwd: null argument");
  if (n < 1 || n > ((size_t)1 << 40)) return fail(HIM_E_INVALID, "bw_pair_bwd: n=%zu", n);
  if (kind != 0 && kind != 1) return fail(HIM_E_INVALID, "bw_pair_bwd: kind %d (0 bce, 1 l1)", kind);
  if (bw_bad_shape(amp, sigma)) return fail(HIM_E_INVALID, "bw_pair_bwd: amp=%g sigma=%g", (double)amp, (double)sigma);
  hipLaunchKernelGGL(bw_pair_bwd_kernel, dim3(bw_bwd_blocks((long long)n)), dim3(256), 0, ST, p, t, dist2, g, sum_w, dp,
                     (long long)n, kind, amp, bw_den(sigma));
  return check_launch("bw_pair_bwd");
}

int him_surface_fwd(const float* p, const float* t, const int* d2_fg, const int* d2_bg, int B, int H, int W, float* out,
                    void* ws, size_t ws_bytes, void* stream) {
  if (!p || !t || !d2_fg || !d2_bg || !out) return fail(HIM_E_INVALID, "surface: null argument");
  if (B < 1 || H < 1 || W < 1) return fail(HIM_E_INVALID, "surface: B=%d H=%d W=%d", B, H, W);
  if (int rc = bw_ws_check("surface", ws, ws_bytes)) return rc;
  const long long n = (long long)B * H * W;
  const int nb = bw_fwd_blocks(n);
  hipLaunchKernelGGL(surface_stage1, dim3(nb), dim3(256), 0, ST, p, t, d2_fg, d2_bg, (double*)ws, n);
  hipLaunchKernelGGL(bw_stage2, dim3(1), dim3(256), 0, ST, (const double*)ws, nb, 0, surface_scale(B, H, W), out);
  return check_launch("surface_fwd");
}

int him_surface_bwd(const float* t, const int* d2_fg, const int* d2_bg, int B, int H, int W, const float* g, float* dp,
                    void* stream) {
  if (!t || !d2_fg || !d2_bg || !g || !dp) return fail(HIM_E_INVALID, "surface_bwd: null argument");
  if (B < 1 || H < 1 || W < 1) return fail(HIM_E_INVALID, "surface_bwd: B=%d H=%d W=%d", B, H, W);
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(surface_bwd_kernel, dim3(bw_bwd_blocks(n)), dim3(256), 0, ST, t, d2_fg, d2_bg, g, dp, n,
                     (float)surface_scale(B, H, W));
  return check_launch("surface_bwd");
}

}  // extern "C"
