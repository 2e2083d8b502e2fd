// Flat-arena Adam, spectral-norm power iteration (forward + full backward), and library metadata.
#include <algorithm>
#include <math.h>

#include "him_common.h"

namespace him {

char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

// torch.optim.Adam single-tensor semantics (torch/optim/adam.py, _single_tensor_adam):
//   exp_avg.lerp_(grad, 1-beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
//   denom = exp_avg_sq.sqrt() / sqrt(bias_correction2) + eps;  param.addcdiv_(exp_avg, denom, value=-lr/bc1)
// Exponential moving average in lerp form: ema' = ema + w * (p - ema), w = 1 - decay rounded to fp32 ONCE by the caller
// (d * ema + (1 - d) * p loses the whole update at d = 0.999 in fp32).  The subtraction and the FMA are spelled out so that
// contraction cannot regroup them; w == 1 (decay 0) stores p itself -- a copy, not a lerp that rounds twice.
__device__ __forceinline__ float ema_lerp(float ema, float p, float w) {
  return w == 1.f ? p : __fmaf_rn(w, __fsub_rn(p, ema), ema);
}

// ONE body for him_adam_step (EMA = false) and him_adam_ema_step (EMA = true): the Adam arithmetic is the same source, so
// p, m, v of the two entries agree bit for bit; the EMA form adds one read and one write of the shadow value (36 instead
// of 28 B per parameter) to the same pass.
// GUARD = true is him_adam_guarded_step: the same body behind two values read from the device, `st` of him_grad_stats.
// st[1] > 0 (a non-finite gradient element somewhere in the arena): every thread returns before its first store.
// st[3] = the clip coefficient c as an fp32 value: the gradient enters the body as fl32(g * c), the multiply skipped at
// c == 1 so that an unclipped guarded step has the bits of the unguarded one.  g itself is only read.
template <bool EMA, bool GUARD>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, float* __restrict__ ema, size_t n, float w1, float beta2,
                            float one_m_beta2, float bc2_sqrt, float eps, float step_size, float ema_w,
                            const double* __restrict__ st) {
  float c = 1.f;
  if (GUARD) {
    if (st[1] > 0.0) return;
    c = (float)st[3];
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float gi = g[i];
    if (GUARD && c != 1.f) gi = __fmul_rn(gi, c);
    float mi = m[i];
    // at::lerp: weight < 0.5 ? start + weight*(end-start) : end - (end-start)*(1-weight)
    const float diff = gi - mi;
    mi = w1 < 0.5f ? mi + w1 * diff : gi - diff * (1.f - w1);
    float vi = v[i] * beta2;
    vi = vi + one_m_beta2 * (gi * gi);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float pi = p[i] - step_size * (mi / denom);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (EMA) ema[i] = ema_lerp(ema[i], pi, ema_w);
  }
}

__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n, float ema_w) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    ema[i] = ema_lerp(ema[i], p[i], ema_w);
}

__global__ void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float t = a[i];
    a[i] = b[i];
    b[i] = t;
  }
}

// ---- gradient statistics (him_grad_stats) ------------------------------------------------------------------------------
// Decomposition, a function of (n, seg) alone: [0, n) is cut into R = 2 * nseg + 1 RANGES -- gap 0, segment 0, gap 1, ...,
// segment nseg-1, tail gap (any of them may be empty) -- and every range into CHUNKS of GS_CHUNK floats counted from the
// range's own start.  One workgroup sums one chunk (element k of the chunk belongs to thread (k / 4) % 256, whatever the
// pointer's alignment; each thread adds its squares in index order into four double lanes, the lanes and the threads meet
// in a fixed tree).  The finish adds the chunk partials of a segment, and of the whole list, in a fixed order.  Neither
// grid size enters: both kernels stride over work items, and an item's value does not depend on which workgroup ran it.
constexpr int GS_CHUNK = 16384;

struct GsWork {
  long long start, len;
};

// workspace: [ranges: R x (begin, len)] [first chunk of range r: R + 1] [work list: cap] [partials: cap x (sum, count)]
struct GsLayout {
  long long R, cap;
  long long* rng;
  long long* first;
  GsWork* work;
  double* part;
};
inline size_t gs_bytes(size_t n, int nseg) {
  const size_t R = 2 * (size_t)nseg + 1, cap = n / GS_CHUNK + R;
  return 8 + (2 * R + (R + 1)) * sizeof(long long) + cap * (sizeof(GsWork) + 2 * sizeof(double));
}
inline GsLayout gs_layout(void* ws, size_t n, int nseg) {
  GsLayout L;
  L.R = 2 * (long long)nseg + 1;
  L.cap = (long long)(n / GS_CHUNK) + L.R;
  L.rng = (long long*)(((uintptr_t)ws + 7) & ~(uintptr_t)7);
  L.first = L.rng + 2 * L.R;
  L.work = (GsWork*)(L.first + L.R + 1);
  L.part = (double*)(L.work + L.cap);
  return L;
}

__device__ __forceinline__ long long gs_clamp(long long x, long long lo, long long hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}
// segment i clamped into [0, n] (a table that breaks its contract gives wrong sums, never an address outside g or ws)
__device__ __forceinline__ void gs_seg(const long long* __restrict__ seg, long long n, long long i, long long& b,
                                       long long& e) {
  b = gs_clamp(seg[2 * i], 0, n);
  e = b + gs_clamp(seg[2 * i + 1], 0, n - b);
}
__device__ __forceinline__ void gs_range(const long long* __restrict__ seg, long long nseg, long long n, long long r,
                                         long long& b, long long& len) {
  long long e;
  if (r & 1) {
    gs_seg(seg, n, r >> 1, b, e);
  } else {
    const long long i = r >> 1;
    long long pb = 0, pe = 0;
    if (i > 0) gs_seg(seg, n, i - 1, pb, pe);
    b = pe;
    if (i < nseg) {
      long long nb, ne;
      gs_seg(seg, n, i, nb, ne);
      e = nb > b ? nb : b;
    } else {
      e = n;
    }
  }
  len = e - b;
}

// one workgroup: the range table, the first chunk index of every range (an integer scan) and the chunk work list
__global__ __launch_bounds__(256) void gs_plan_kernel(const long long* __restrict__ seg, long long nseg, long long n,
                                                      long long R, long long cap, long long* __restrict__ rng,
                                                      long long* __restrict__ first, GsWork* __restrict__ work) {
  __shared__ long long sh[257];
  const int t = threadIdx.x;
  const long long per = (R + 255) / 256;
  const long long r0 = t * per, r1 = r0 + per < R ? r0 + per : R;
  long long mine = 0;
  for (long long r = r0; r < r1; ++r) {
    long long b, len;
    gs_range(seg, nseg, n, r, b, len);
    rng[2 * r] = b;
    rng[2 * r + 1] = len;
    mine += (len + GS_CHUNK - 1) / GS_CHUNK;
  }
  sh[t + 1] = mine;
  __syncthreads();
  if (t == 0) {
    sh[0] = 0;
    for (int k = 1; k <= 256; ++k) sh[k] += sh[k - 1];
  }
  __syncthreads();
  long long w = sh[t];
  for (long long r = r0; r < r1; ++r) {
    long long b, len;
    gs_range(seg, nseg, n, r, b, len);
    first[r] = w < cap ? w : cap;
    for (long long o = 0; o < len; o += GS_CHUNK, ++w)
      if (w < cap) {
        work[w].start = b + o;
        work[w].len = len - o < GS_CHUNK ? len - o : GS_CHUNK;
      }
  }
  if (t == 255) first[R] = sh[256] < cap ? sh[256] : cap;
}

// finite: x * x is exact in double (24 x 24 bits) and the fma rounds the sum once; Inf / NaN: counted, adds nothing
__device__ __forceinline__ void gs_acc(float x, double& acc, unsigned& bad) {
  if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {
    ++bad;
  } else {
    const double d = (double)x;
    acc = fma(d, d, acc);
  }
}

__global__ __launch_bounds__(256) void gs_partial_kernel(const float* __restrict__ g, const GsWork* __restrict__ work,
                                                         const long long* __restrict__ first, long long R,
                                                         double* __restrict__ part) {
  __shared__ double sh[4];
  const long long total = first[R];
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const float* __restrict__ src = g + work[w].start;
    const int len = (int)work[w].len;
    const bool wide = ((uintptr_t)src & 15) == 0;      // uniform over the workgroup
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    unsigned bad = 0;
    for (int k = 4 * (int)threadIdx.x; k < len; k += 1024) {
      if (k + 4 <= len) {
        float4 q;
        if (wide) {
          q = *reinterpret_cast<const float4*>(src + k);
        } else {
          q.x = src[k];
          q.y = src[k + 1];
          q.z = src[k + 2];
          q.w = src[k + 3];
        }
        gs_acc(q.x, a0, bad);
        gs_acc(q.y, a1, bad);
        gs_acc(q.z, a2, bad);
        gs_acc(q.w, a3, bad);
      } else {                                         // the chunk's last, partial quad
        gs_acc(src[k], a0, bad);
        if (k + 1 < len) gs_acc(src[k + 1], a1, bad);
        if (k + 2 < len) gs_acc(src[k + 2], a2, bad);
      }
    }
    const double s = block_sum_f64((a0 + a1) + (a2 + a3), sh);
    const double c = block_sum_f64((double)bad, sh);     // <= 16384: exact
    if (threadIdx.x == 0) {
      part[2 * w] = s;
      part[2 * w + 1] = c;
    }
  }
}

// workgroup 0: the whole list -> st.  Workgroups 1..: one wavefront per segment -> seg_out.  Thread (lane) t adds the
// partials t, t + 256 (64), ... in that order, then the fixed tree: independent of how many workgroups the launch has.
__global__ __launch_bounds__(256) void gs_finish_kernel(const double* __restrict__ part,
                                                        const long long* __restrict__ first, long long R, long long nseg,
                                                        double* __restrict__ seg_out, double* __restrict__ st,
                                                        double max_norm) {
  __shared__ double sh[4];
  if (blockIdx.x == 0) {
    const long long total = first ? first[R] : 0;
    double s = 0.0, c = 0.0;
    for (long long w = threadIdx.x; w < total; w += 256) {
      s += part[2 * w];
      c += part[2 * w + 1];
    }
    s = block_sum_f64(s, sh);
    c = block_sum_f64(c, sh);
    if (threadIdx.x == 0) {
      const double nrm = sqrt(s);
      float coef = 1.f;
      if (max_norm > 0.0 && max_norm < INFINITY) {
        const double q = max_norm / (nrm + 1e-6);
        coef = (float)(q < 1.0 ? q : 1.0);
      }
      const double calls = st[4], skipped = st[5];
      st[0] = s;
      st[1] = c;
      st[2] = nrm;
      st[3] = (double)coef;
      st[4] = calls + 1.0;
      st[5] = skipped + (c > 0.0 ? 1.0 : 0.0);
      st[6] = 0.0;
      st[7] = 0.0;
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  for (long long i = ((long long)blockIdx.x - 1) * 4 + (threadIdx.x >> 6); i < nseg; i += ((long long)gridDim.x - 1) * 4) {
    double s = 0.0, c = 0.0;
    if (first) {
      const long long w1 = first[2 * i + 2];
      for (long long w = first[2 * i + 1] + lane; w < w1; w += 64) {
        s += part[2 * w];
        c += part[2 * w + 1];
      }
    }
    s = wave_sum_f64(s);
    c = wave_sum_f64(c);
    if (lane == 0) {
      seg_out[2 * i] = s;
      seg_out[2 * i + 1] = c;
    }
  }
}

// ---- spectral norm -----------------------------------------------------------------------------
// s_j = sum_i u_i W_ij   (coalesced over j)
__global__ void sn_colsum_kernel(const float* __restrict__ W, const float* __restrict__ u, int rows, int cols,
                                 float* __restrict__ s) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  float acc = 0.f;
  for (int i = 0; i < rows; ++i) acc += u[i] * W[(size_t)i * cols + j];
  s[j] = acc;
}
// t_i = sum_j W_ij v_j   (one 256-thread block per row)
__global__ __launch_bounds__(256) void sn_rowdot_kernel(const float* __restrict__ W, const float* __restrict__ v,
                                                        int cols, float* __restrict__ t) {
  __shared__ float sh[8];
  const int i = blockIdx.x;
  float acc = 0.f;
  for (int j = threadIdx.x; j < cols; j += 256) acc += W[(size_t)i * cols + j] * v[j];
  acc = block_sum_256(acc, sh);
  if (threadIdx.x == 0) t[i] = acc;
}
// out = in / (||in|| + eps)   single block
__global__ __launch_bounds__(256) void sn_l2n_kernel(const float* __restrict__ in, int n, float eps,
                                                     float* __restrict__ out) {
  __shared__ float sh[8];
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) q += in[i] * in[i];
  const float nrm = sqrtf(block_sum_256(q, sh));
  for (int i = threadIdx.x; i < n; i += 256) out[i] = in[i] / (nrm + eps);
}
// u' = t/(|t|+eps), sigma = u'.t
__global__ __launch_bounds__(256) void sn_finish_kernel(const float* __restrict__ t, int n, float eps,
                                                        float* __restrict__ u_out, float* __restrict__ sigma) {
  __shared__ float sh[8];
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) q += t[i] * t[i];
  const float nrm = sqrtf(block_sum_256(q, sh));
  float d = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float ui = t[i] / (nrm + eps);
    u_out[i] = ui;
    d += ui * t[i];
  }
  d = block_sum_256(d, sh);
  if (threadIdx.x == 0) sigma[0] = d;
}
// a = t/(|t|+eps) + t*eps/(|t|+eps)^2   (d sigma / d (W v) including the path through u')
__global__ __launch_bounds__(256) void sn_bwd_a_kernel(const float* __restrict__ t, int n, float eps,
                                                       float* __restrict__ a) {
  __shared__ float sh[8];
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) q += t[i] * t[i];
  const float nrm = sqrtf(block_sum_256(q, sh));
  const float d = nrm + eps;
  for (int i = threadIdx.x; i < n; i += 256) a[i] = t[i] / d + t[i] * (eps / (d * d));
}
// ds = dv/(|s|+eps) - s (s.dv)/(|s| (|s|+eps)^2)
__global__ __launch_bounds__(256) void sn_bwd_ds_kernel(const float* __restrict__ s, const float* __restrict__ dv,
                                                        int n, float eps, float* __restrict__ ds) {
  __shared__ float sh[8];
  float q = 0.f, d = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    q += s[i] * s[i];
    d += s[i] * dv[i];
  }
  const float nrm = sqrtf(block_sum_256(q, sh));
  d = block_sum_256(d, sh);
  const float den = nrm + eps;
  const float k = nrm > 0.f ? d / (nrm * den * den) : 0.f;
  for (int i = threadIdx.x; i < n; i += 256) ds[i] = dv[i] / den - s[i] * k;
}
__global__ void sn_bwd_dw_kernel(const float* __restrict__ a, const float* __restrict__ v,
                                 const float* __restrict__ u, const float* __restrict__ ds,
                                 const float* __restrict__ g, int rows, int cols, float* __restrict__ dW,
                                 int accumulate) {
  const size_t n = (size_t)rows * cols;
  const float gs = g[0];
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / cols), j = (int)(idx % cols);
    const float val = gs * (a[i] * v[j] + u[i] * ds[j]);
    dW[idx] = accumulate ? dW[idx] + val : val;
  }
}

__global__ void div_scalar_fwd_kernel(const float* __restrict__ W, const float* __restrict__ sigma,
                                      float* __restrict__ out, size_t n) {
  const float s = sigma[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = W[i] / s;
}
__global__ __launch_bounds__(256) void div_scalar_bwd1_kernel(const float* __restrict__ W,
                                                              const float* __restrict__ sigma,
                                                              const float* __restrict__ dout, float* __restrict__ dW,
                                                              float* __restrict__ partial, size_t n, int accumulate) {
  __shared__ float sh[8];
  const float s = sigma[0];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float d = dout[i];
    acc += d * W[i];
    const float val = d / s;
    dW[i] = accumulate ? dW[i] + val : val;
  }
  acc = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void div_scalar_bwd2_kernel(const float* __restrict__ partial, int nb,
                                                              const float* __restrict__ sigma,
                                                              float* __restrict__ dsigma) {
  __shared__ float sh[8];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  acc = block_sum_256(acc, sh);
  if (threadIdx.x == 0) dsigma[0] = -acc / (sigma[0] * sigma[0]);
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

// Shared front end of him_adam_step / him_adam_ema_step: the hyper-parameters arrive as the DOUBLES the caller holds
// (python floats), exactly as torch.optim.Adam sees them: torch derives 1 - beta2, the bias corrections and lr / bc1 in
// double and only then rounds each scalar to fp32 (round 2 took floats: 1.f - 0.999f = 1.0000467e-3 instead of 1e-3, a
// 4.7e-5 relative bias of exp_avg_sq).
template <bool EMA, bool GUARD = false>
static int adam_launch(const char* what, float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr,
                       double beta1, double beta2, double eps, int step, double ema_decay, void* stream,
                       const double* st = nullptr) {
  if (step < 1) return fail(HIM_E_INVALID, "adam: step must be >= 1");
  if (EMA && !(ema_decay >= 0.0 && ema_decay < 1.0)) return fail(HIM_E_INVALID, "adam_ema: ema_decay outside [0, 1)");
  if (!n) return HIM_OK;
  if (!p || !g || !m || !v || (EMA && !ema) || (GUARD && !st)) return fail(HIM_E_INVALID, "adam: null pointer");
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const int nb = (int)std::min<size_t>((n + 255) / 256, 256 * 16);
  hipLaunchKernelGGL((adam_kernel<EMA, GUARD>), dim3(nb), dim3(256), 0, ST, p, g, m, v, ema, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), bc2_sqrt, (float)eps, step_size, (float)(1.0 - ema_decay), st);
  return check_launch(what);
}

extern "C" {

const char* him_version(void) { return "him-hip 0.6 (round 6)"; }
const char* him_arch(void) { return "gfx950"; }
const char* him_last_error(void) { return err_buf(); }

int him_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2,
                  double eps, int step, void* stream) {
  if (!n) return HIM_OK;
  return adam_launch<false>("adam", p, g, m, v, nullptr, n, lr, beta1, beta2, eps, step, 0.0, stream);
}

int him_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double beta1,
                      double beta2, double eps, int step, double ema_decay, void* stream) {
  return adam_launch<true>("adam_ema", p, g, m, v, ema, n, lr, beta1, beta2, eps, step, ema_decay, stream);
}

int him_ema_update(float* ema, const float* p, size_t n, double ema_decay, void* stream) {
  if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return fail(HIM_E_INVALID, "ema_update: ema_decay outside [0, 1)");
  if (!n) return HIM_OK;
  if (!ema || !p) return fail(HIM_E_INVALID, "ema_update: null pointer");
  const int nb = (int)std::min<size_t>((n + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(ema_kernel, dim3(nb), dim3(256), 0, ST, ema, p, n, (float)(1.0 - ema_decay));
  return check_launch("ema_update");
}

int him_swap(float* a, float* b, size_t n, void* stream) {
  if (!n) return HIM_OK;
  if (!a || !b) return fail(HIM_E_INVALID, "swap: null pointer");
  const int nb = (int)std::min<size_t>((n + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(swap_kernel, dim3(nb), dim3(256), 0, ST, a, b, n);
  return check_launch("swap");
}

size_t him_grad_stats_ws(size_t n, int nseg) { return gs_bytes(n, nseg < 0 ? 0 : nseg); }

int him_grad_stats(const float* g, size_t n, const long long* seg, int nseg, double* seg_out, double* st,
                   double max_norm, void* ws, size_t ws_bytes, void* stream) {
  if (nseg < 0) return fail(HIM_E_INVALID, "grad_stats: nseg < 0");
  if (!(max_norm >= 0.0)) return fail(HIM_E_INVALID, "grad_stats: max_norm is negative or NaN");
  if (!st) return fail(HIM_E_INVALID, "grad_stats: null st");
  if (nseg > 0 && (!seg || !seg_out)) return fail(HIM_E_INVALID, "grad_stats: null segment table");
  if (n > 0 && (!g || !ws)) return fail(HIM_E_INVALID, "grad_stats: null pointer");
  if (n > 0 && ws_bytes < gs_bytes(n, nseg)) return fail(HIM_E_WORKSPACE, "grad_stats: ws too small");
  const int nfin = 1 + (int)std::min<long long>(((long long)nseg + 3) / 4, 1024);
  if (!n) {      // nothing to read: zeros everywhere, the call still counts
    hipLaunchKernelGGL(gs_finish_kernel, dim3(nfin), dim3(256), 0, ST, (const double*)nullptr,
                       (const long long*)nullptr, (long long)0, (long long)nseg, seg_out, st, max_norm);
    return check_launch("grad_stats");
  }
  const GsLayout L = gs_layout(ws, n, nseg);
  hipLaunchKernelGGL(gs_plan_kernel, dim3(1), dim3(256), 0, ST, seg, (long long)nseg, (long long)n, L.R, L.cap, L.rng,
                     L.first, L.work);
  hipLaunchKernelGGL(gs_partial_kernel, dim3((unsigned)std::min<long long>(L.cap, 1 << 20)), dim3(256), 0, ST, g,
                     (const GsWork*)L.work, (const long long*)L.first, L.R, L.part);
  hipLaunchKernelGGL(gs_finish_kernel, dim3(nfin), dim3(256), 0, ST, (const double*)L.part, (const long long*)L.first,
                     L.R, (long long)nseg, seg_out, st, max_norm);
  return check_launch("grad_stats");
}

int him_adam_guarded_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double beta1,
                          double beta2, double eps, int step, double ema_decay, const double* st, void* stream) {
  if (ema) return adam_launch<true, true>("adam_guarded", p, g, m, v, ema, n, lr, beta1, beta2, eps, step, ema_decay, stream, st);
  return adam_launch<false, true>("adam_guarded", p, g, m, v, nullptr, n, lr, beta1, beta2, eps, step, 0.0, stream, st);
}

size_t him_sn_ws(int rows, int cols) { return ((size_t)2 * rows + 3 * (size_t)cols + 64) * sizeof(float); }

int him_sn_power_iter_fwd(const float* W, const float* u, int rows, int cols, float* v_out, float* u_out,
                          float* sigma_out, void* ws, size_t ws_bytes, void* stream) {
  if (rows <= 0 || cols <= 0) return fail(HIM_E_INVALID, "sn: bad shape");
  if (!W || !u || !v_out || !u_out || !sigma_out) return fail(HIM_E_INVALID, "sn: null pointer");
  if (!ws || ws_bytes < him_sn_ws(rows, cols)) return fail(HIM_E_WORKSPACE, "sn: ws too small");
  float* t = (float*)ws;
  float* s = t + 2 * rows;
  hipLaunchKernelGGL(sn_colsum_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, ST, W, u, rows, cols, s);
  hipLaunchKernelGGL(sn_l2n_kernel, dim3(1), dim3(256), 0, ST, (const float*)s, cols, 1e-12f, v_out);
  hipLaunchKernelGGL(sn_rowdot_kernel, dim3(rows), dim3(256), 0, ST, W, (const float*)v_out, cols, t);
  hipLaunchKernelGGL(sn_finish_kernel, dim3(1), dim3(256), 0, ST, (const float*)t, rows, 1e-12f, u_out, sigma_out);
  return check_launch("sn_fwd");
}

int him_sn_power_iter_bwd(const float* W, const float* u, const float* v_out, const float* u_out, const float* sigma,
                          const float* g_sigma, int rows, int cols, float* dW, int accumulate, void* ws,
                          size_t ws_bytes, void* stream) {
  (void)u_out;
  (void)sigma;
  if (rows <= 0 || cols <= 0) return fail(HIM_E_INVALID, "sn: bad shape");
  if (!W || !u || !v_out || !g_sigma || !dW) return fail(HIM_E_INVALID, "sn: null pointer");
  if (!ws || ws_bytes < him_sn_ws(rows, cols)) return fail(HIM_E_WORKSPACE, "sn: ws too small");
  float* t = (float*)ws;
  float* a = t + rows;
  float* s = a + rows;
  float* dv = s + cols;
  float* ds = dv + cols;
  hipLaunchKernelGGL(sn_rowdot_kernel, dim3(rows), dim3(256), 0, ST, W, v_out, cols, t);
  hipLaunchKernelGGL(sn_bwd_a_kernel, dim3(1), dim3(256), 0, ST, (const float*)t, rows, 1e-12f, a);
  hipLaunchKernelGGL(sn_colsum_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, ST, W, (const float*)a, rows, cols, dv);
  hipLaunchKernelGGL(sn_colsum_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, ST, W, u, rows, cols, s);
  hipLaunchKernelGGL(sn_bwd_ds_kernel, dim3(1), dim3(256), 0, ST, (const float*)s, (const float*)dv, cols, 1e-12f, ds);
  const size_t n = (size_t)rows * cols;
  hipLaunchKernelGGL(sn_bwd_dw_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, ST,
                     (const float*)a, v_out, u, (const float*)ds, g_sigma, rows, cols, dW, accumulate);
  return check_launch("sn_bwd");
}

int him_div_scalar_fwd(const float* W, const float* sigma, float* out, size_t n, void* stream) {
  if (!n) return HIM_OK;
  if (!W || !sigma || !out) return fail(HIM_E_INVALID, "div_scalar: null pointer");
  hipLaunchKernelGGL(div_scalar_fwd_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0,
                     ST, W, sigma, out, n);
  return check_launch("div_scalar_fwd");
}

int him_div_scalar_bwd(const float* W, const float* sigma, const float* dout, float* dW, float* dsigma, size_t n,
                       int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (!n) return HIM_OK;
  if (!W || !sigma || !dout || !dW || !dsigma) return fail(HIM_E_INVALID, "div_scalar: null pointer");
  const int nb = (int)std::min<size_t>((n + 1023) / 1024, 1024);   // min(ceil(n / 1024), 1024) partial sums: include/him.h
  if (!ws || ws_bytes < (size_t)nb * sizeof(float)) return fail(HIM_E_WORKSPACE, "div_scalar: ws too small");
  hipLaunchKernelGGL(div_scalar_bwd1_kernel, dim3(nb), dim3(256), 0, ST, W, sigma, dout, dW, (float*)ws, n,
                     accumulate);
  hipLaunchKernelGGL(div_scalar_bwd2_kernel, dim3(1), dim3(256), 0, ST, (const float*)ws, nb, sigma, dsigma);
  return check_launch("div_scalar_bwd");
}

}  // extern "C"
