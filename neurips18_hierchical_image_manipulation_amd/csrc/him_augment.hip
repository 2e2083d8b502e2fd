// Differentiable discriminator augmentation (him_diffaug_*): colour -> translation (zero fill) -> cutout on the dense
// (B, C, H, W) discriminator input, its exact adjoint, and the stateless parameter draw.  Semantics: include/him.h.
//
// Layout of the two tensor passes.  grid.y strides over (sample, channel) planes, so everything read from the parameter
// table is uniform over a workgroup; grid.x strides over the plane's QUADS: four consecutive columns of one row.  A quad
// is one 16-byte load and one 16-byte store when it lies inside the row on both sides; the vector type is declared with
// 4-byte alignment, so a shift that is no multiple of 4, a width that is no multiple of 4 and a base pointer that is only
// 4-byte aligned all take the same path (gfx950 global accesses need dword alignment only).  A quad that crosses the
// plane's edge on the source side, and the partial quad behind a row whose width is no multiple of 4, go element by
// element; nothing else does.  The three image channels of a colour row are done by ONE work item (the plane of the first
// image channel in range; the other two planes return at once), which reads each source value once.
//
// Reductions (the per-sample sum of the image channels, and of the routed gradient): him_grad_stats' rule.  The 3*H*W
// contiguous floats of a sample are cut into chunks of DA_CHUNK counted from the sample's first image element; one
// workgroup adds one chunk (element k belongs to thread (k / 4) % 256, four double lanes per thread, fixed tree), a second
// launch adds a sample's chunk partials (thread t takes t, t + 256, ..., fixed tree).  No atomics, and neither grid size
// enters the value.
#include "him_common.h"

namespace him {

constexpr int DA_CHUNK = 16384;
constexpr int DA_COLOR = 1, DA_TRANSLATE = 2, DA_CUTOUT = 4;

typedef float da_f4 __attribute__((ext_vector_type(4), aligned(4)));

// one sample's row of the table, clamped so that no content can move an address out of the plane
struct DaRow {
  float b, a, k;
  int ty, tx;              // in [-H, H] / [-W, W]
  int cy0, cy1, cx0, cx1;  // the cutout intersected with the plane, [cy0, cy1) x [cx0, cx1); empty: all 0
  int bits;
};

__device__ __forceinline__ int da_clamp(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

__device__ __forceinline__ DaRow da_row(const int* __restrict__ table, int b, int H, int W, int ch, int cw, int policy) {
  const int* r = table + 8 * (size_t)b;
  DaRow o;
  o.bits = r[7] & policy;
  o.b = __int_as_float(r[0]);
  o.a = __int_as_float(r[1]);
  o.k = __int_as_float(r[2]);
  o.ty = o.tx = 0;
  if (o.bits & DA_TRANSLATE) {
    o.ty = da_clamp(r[3], -H, H);
    o.tx = da_clamp(r[4], -W, W);
  }
  o.cy0 = o.cy1 = o.cx0 = o.cx1 = 0;
  if (o.bits & DA_CUTOUT) {
    const int y0 = da_clamp(r[5], 0, H), y1 = da_clamp((long long)r[5] + ch, 0, H);
    const int x0 = da_clamp(r[6], 0, W), x1 = da_clamp((long long)r[6] + cw, 0, W);
    if (y1 > y0 && x1 > x0) {
      o.cy0 = y0;
      o.cy1 = y1;
      o.cx0 = x0;
      o.cx1 = x1;
    }
  }
  return o;
}

// Four columns x0 .. x0+3 of destination row y of one plane, gathered from `src` (the same plane of the other tensor):
// forward  (FWD):  out[y][x] = in[y + ty][x + tx], zero outside the plane or where (y, x) is cut;
// backward (!FWD): g[y][x]   = dout[y - ty][x - tx], zero outside the plane or where that OUTPUT position is cut.
// Lanes at or behind column W stay zero.
template <bool FWD>
__device__ __forceinline__ void da_gather(const float* __restrict__ src, const DaRow& r, int H, int W, int y, int x0,
                                          float v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  const int sy = FWD ? r.ty : -r.ty, sx = FWD ? r.tx : -r.tx;
  const int ys = y + sy;                       // |ty| <= H: no overflow
  if (ys < 0 || ys >= H) return;
  const int yc = FWD ? y : ys;                 // the row of the OUTPUT position
  const bool row_cut = yc >= r.cy0 && yc < r.cy1;
  const int xs0 = x0 + sx;
  const int xc0 = FWD ? x0 : xs0;
  if (row_cut && xc0 >= r.cx0 && xc0 + 4 <= r.cx1) return;      // the whole quad is cut: nothing is read
  const float* __restrict__ row = src + (size_t)ys * W;
  if (xs0 >= 0 && xs0 + 4 <= W && x0 + 4 <= W) {
    const da_f4 q = *reinterpret_cast<const da_f4*>(row + xs0);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xs = xs0 + j;
      if (x0 + j < W && xs >= 0 && xs < W) v[j] = row[xs];
    }
  }
  if (row_cut) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (xc0 + j >= r.cx0 && xc0 + j < r.cx1) v[j] = 0.f;
  }
}

__device__ __forceinline__ void da_store(float* __restrict__ row, int W, int x0, const float v[4]) {
  if (x0 + 4 <= W) {
    da_f4 q;
    q.x = v[0];
    q.y = v[1];
    q.z = v[2];
    q.w = v[3];
    *reinterpret_cast<da_f4*>(row + x0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < W) row[x0 + j] = v[j];
  }
}

// src (B, C, H, W) -> dst (B, gn, H, W) holding channels [g0, g0 + gn) (forward: g0 = 0, gn = C).
template <bool FWD>
__global__ __launch_bounds__(256) void da_apply_kernel(const float* __restrict__ src, const int* __restrict__ table,
                                                       float* __restrict__ dst, const double* __restrict__ sums, int B,
                                                       int C, int c0, int H, int W, int ch, int cw, int policy, int g0,
                                                       int gn) {
  const int Q = (W + 3) >> 2;
  const unsigned nquad = (unsigned)H * (unsigned)Q;
  const size_t hw = (size_t)H * W;
  const long long planes = (long long)B * gn;
  for (long long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int b = (int)(pl / gn), c = g0 + (int)(pl % gn);
    const DaRow r = da_row(table, b, H, W, ch, cw, policy);
    const bool image = (r.bits & DA_COLOR) && c >= c0 && c < c0 + 3;
    if (!image) {
      const float* __restrict__ sp = src + ((size_t)b * C + c) * hw;
      float* __restrict__ dp = dst + ((size_t)b * gn + (c - g0)) * hw;
      for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < nquad; j += gridDim.x * 256u) {
        const int y = (int)(j / (unsigned)Q), x0 = (int)(j % (unsigned)Q) * 4;
        float v[4];
        da_gather<FWD>(sp, r, H, W, y, x0, v);
        da_store(dp + (size_t)y * W, W, x0, v);
      }
      continue;
    }
    // colour row: the first image channel in range does every image channel in range
    const int lo = c0 > g0 ? c0 : g0, hi = c0 + 3 < g0 + gn ? c0 + 3 : g0 + gn;
    if (c != lo) continue;
    const float* __restrict__ sp = src + ((size_t)b * C + c0) * hw;
    float* __restrict__ dp = dst + (size_t)b * gn * hw;
    const double n3 = 3.0 * (double)hw;
    const float t = (float)(sums[b] / n3);       // forward: the mean of x; backward: S_b / N
    const float m = t + r.b;
    const float omk = 1.f - r.k, oma = 1.f - r.a;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < nquad; j += gridDim.x * 256u) {
      const int y = (int)(j / (unsigned)Q), x0 = (int)(j % (unsigned)Q) * 4;
      float v0[4], v1[4], v2[4];
      da_gather<FWD>(sp, r, H, W, y, x0, v0);
      da_gather<FWD>(sp + hw, r, H, W, y, x0, v1);
      da_gather<FWD>(sp + 2 * hw, r, H, W, y, x0, v2);
      if (FWD) {
        // which lanes hold a routed value (the others stay zero: outside the plane, or cut)
        const int ys = y + r.ty;
        const bool row_in = ys >= 0 && ys < H;
        const bool row_cut = y >= r.cy0 && y < r.cy1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int x = x0 + q, xs = x + r.tx;
          const bool live = row_in && xs >= 0 && xs < W && !(row_cut && x >= r.cx0 && x < r.cx1);
          const float a0 = v0[q] + r.b, a1 = v1[q] + r.b, a2 = v2[q] + r.b;
          const float p = (a0 + a1 + a2) / 3.f;
          const float s0 = (a0 - p) * r.a + p, s1 = (a1 - p) * r.a + p, s2 = (a2 - p) * r.a + p;
          v0[q] = live ? (s0 - m) * r.k + m : 0.f;
          v1[q] = live ? (s1 - m) * r.k + m : 0.f;
          v2[q] = live ? (s2 - m) * r.k + m : 0.f;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float d0 = r.k * v0[q] + omk * t, d1 = r.k * v1[q] + omk * t, d2 = r.k * v2[q] + omk * t;
          const float dm = (d0 + d1 + d2) / 3.f;
          v0[q] = r.a * d0 + oma * dm;
          v1[q] = r.a * d1 + oma * dm;
          v2[q] = r.a * d2 + oma * dm;
        }
      }
      float* __restrict__ orow = dp + (size_t)y * W;       // channel g0's row y; image channel i is (c0 + i - g0) planes on
      if (c0 >= lo && c0 < hi) da_store(orow + (size_t)(c0 - g0) * hw, W, x0, v0);
      if (c0 + 1 >= lo && c0 + 1 < hi) da_store(orow + (size_t)(c0 + 1 - g0) * hw, W, x0, v1);
      if (c0 + 2 >= lo && c0 + 2 < hi) da_store(orow + (size_t)(c0 + 2 - g0) * hw, W, x0, v2);
    }
  }
}

// part[b * nchunk + j] = sum of chunk j of sample b's three image channels.  Forward: every element.  Backward: the
// elements of dout that the forward pass routed somewhere (source inside the plane, not cut).  A sample whose row has no
// colour bit is not read: its partials are zero.
template <bool FWD>
__global__ __launch_bounds__(256) void da_partial_kernel(const float* __restrict__ src, const int* __restrict__ table,
                                                         double* __restrict__ part, int B, int C, int c0, int H, int W,
                                                         int ch, int cw, int policy, int nchunk) {
  __shared__ double sh[4];
  const size_t hw = (size_t)H * W;
  const long long n = 3 * (long long)hw, total = (long long)B * nchunk;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const int b = (int)(w / nchunk);
    const long long k0 = (w % nchunk) * (long long)DA_CHUNK;
    const DaRow r = da_row(table, b, H, W, ch, cw, policy);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (r.bits & DA_COLOR) {
      const float* __restrict__ p = src + ((size_t)b * C + c0) * hw + k0;
      const int len = (int)(n - k0 < DA_CHUNK ? n - k0 : DA_CHUNK);
      for (int k = 4 * (int)threadIdx.x; k < len; k += 1024) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (k + 4 <= len) {
          const da_f4 q = *reinterpret_cast<const da_f4*>(p + k);
          v[0] = q.x;
          v[1] = q.y;
          v[2] = q.z;
          v[3] = q.w;
        } else {
          v[0] = p[k];
          if (k + 1 < len) v[1] = p[k + 1];
          if (k + 2 < len) v[2] = p[k + 2];
        }
        if (!FWD) {
          const unsigned e0 = (unsigned)((k0 + k) % (long long)hw);      // position inside its plane (3 * hw < 2^31)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned e = (e0 + (unsigned)j) % (unsigned)hw;          // may run into the next image channel's plane
            const int y = (int)(e / (unsigned)W), x = (int)(e % (unsigned)W);
            const int ys = y + r.ty, xs = x + r.tx;
            const bool inside = ys >= 0 && ys < H && xs >= 0 && xs < W;
            const bool cut = y >= r.cy0 && y < r.cy1 && x >= r.cx0 && x < r.cx1;
            v[j] = (inside && !cut) ? v[j] : 0.f;
          }
        }
        a0 += (double)v[0];
        a1 += (double)v[1];
        a2 += (double)v[2];
        a3 += (double)v[3];
      }
    }
    const double s = block_sum_f64((a0 + a1) + (a2 + a3), sh);
    if (threadIdx.x == 0) part[w] = s;
  }
}

__global__ __launch_bounds__(256) void da_finish_kernel(const double* __restrict__ part, double* __restrict__ sums, int B,
                                                        int nchunk) {
  __shared__ double sh[4];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    double s = 0.0;
    for (int j = threadIdx.x; j < nchunk; j += 256) s += part[(size_t)b * nchunk + j];
    s = block_sum_f64(s, sh);
    if (threadIdx.x == 0) sums[b] = s;
  }
}

// ---- the draw ----------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned long long da_mix(unsigned long long z) {     // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr unsigned long long DA_GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ float da_uniform(unsigned long long z) { return (float)(unsigned)(z >> 40) * 0x1p-24f; }
__device__ __forceinline__ int da_randint(unsigned long long z, int lo, int hi) {
  return lo + (int)(((z >> 32) * (unsigned long long)((long long)hi - lo + 1)) >> 32);
}

__global__ void da_draw_kernel(int* __restrict__ table, int B, int H, int W, unsigned long long seed,
                               unsigned long long step, unsigned long long sample0, int policy, int sy, int sx, int ch,
                               int cw) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long key = da_mix(da_mix(da_mix(seed + DA_GOLDEN) + step + DA_GOLDEN) + (sample0 + b) + DA_GOLDEN);
  unsigned long long z[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) z[i] = da_mix(key + (unsigned long long)(i + 1) * DA_GOLDEN);
  float fb = 0.f, fa = 1.f, fk = 1.f;
  int ty = 0, tx = 0, cy = 0, cx = 0;
  if (policy & DA_COLOR) {
    fb = da_uniform(z[0]) - 0.5f;
    fa = da_uniform(z[1]) * 2.f;
    fk = da_uniform(z[2]) + 0.5f;
  }
  if (policy & DA_TRANSLATE) {
    ty = da_randint(z[3], -sy, sy);
    tx = da_randint(z[4], -sx, sx);
  }
  if (policy & DA_CUTOUT) {
    cy = da_randint(z[5], 0, H - (ch & 1)) - ch / 2;
    cx = da_randint(z[6], 0, W - (cw & 1)) - cw / 2;
  }
  int* r = table + 8 * (size_t)b;
  r[0] = __float_as_int(fb);
  r[1] = __float_as_int(fa);
  r[2] = __float_as_int(fk);
  r[3] = ty;
  r[4] = tx;
  r[5] = cy;
  r[6] = cx;
  r[7] = policy & 7;
}

static inline int da_nchunk(int H, int W) { return (int)((3ll * H * W + DA_CHUNK - 1) / DA_CHUNK); }
static inline size_t da_bytes(int B, int H, int W) { return 8 + 8 * (size_t)B * (1 + (size_t)da_nchunk(H, W)); }

static int da_check(const char* who, const void* src, const int* table, const void* dst, int B, int C, int c0, int H,
                    int W, int ch, int cw, int policy, int g0, int gn, const void* ws, size_t ws_bytes) {
  if (!src || !table || !dst) return fail(HIM_E_INVALID, "%s: null pointer", who);
  if (B < 0 || C < 0 || H < 0 || W < 0 || ch < 0 || cw < 0 || c0 < 0) return fail(HIM_E_INVALID, "%s: negative size", who);
  if ((long long)H * W > 0x7fffffffll / 4) return fail(HIM_E_INVALID, "%s: H * W too large", who);
  if (policy & ~7) return fail(HIM_E_INVALID, "%s: unknown policy bits", who);
  if (g0 < 0 || gn < 0 || (long long)g0 + gn > C) return fail(HIM_E_INVALID, "%s: channel range outside [0, C)", who);
  if (policy & DA_COLOR) {
    if ((long long)c0 + 3 > C) return fail(HIM_E_INVALID, "%s: image channels [c0, c0 + 3) outside [0, C)", who);
    if (!ws) return fail(HIM_E_INVALID, "%s: null workspace", who);
    if (ws_bytes < da_bytes(B, H, W)) return fail(HIM_E_INVALID, "%s: workspace smaller than him_diffaug_ws", who);
  }
  return HIM_OK;
}

template <bool FWD>
static int da_run(const char* who, const float* src, const int* table, float* dst, int B, int C, int c0, int H, int W,
                  int ch, int cw, int policy, int g0, int gn, void* ws, size_t ws_bytes, hipStream_t st) {
  const int rc = da_check(who, src, table, dst, B, C, c0, H, W, ch, cw, policy, g0, gn, ws, ws_bytes);
  if (rc != HIM_OK) return rc;
  if (B == 0 || gn == 0 || H == 0 || W == 0) return HIM_OK;
  double* sums = nullptr;
  if (policy & DA_COLOR) {
    const int nchunk = da_nchunk(H, W);
    sums = (double*)(((uintptr_t)ws + 7) & ~(uintptr_t)7);
    double* part = sums + B;
    const long long items = (long long)B * nchunk;
    hipLaunchKernelGGL(da_partial_kernel<FWD>, dim3((unsigned)(items < 4096 ? items : 4096)), dim3(256), 0, st, src,
                       table, part, B, C, c0, H, W, ch, cw, policy, nchunk);
    hipLaunchKernelGGL(da_finish_kernel, dim3((unsigned)(B < 1024 ? B : 1024)), dim3(256), 0, st, part, sums, B, nchunk);
  }
  const long long nquad = (long long)H * ((W + 3) / 4), planes = (long long)B * gn;
  long long gx = (nquad + 255) / 256;
  if (gx > 64) gx = 64;
  const long long gy = planes < 65535 ? planes : 65535;
  hipLaunchKernelGGL(da_apply_kernel<FWD>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, src, table, dst, sums, B, C,
                     c0, H, W, ch, cw, policy, g0, gn);
  return check_launch(who);
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_diffaug_ws(int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0 || (long long)H * W > 0x7fffffffll / 4) return 0;
  return da_bytes(B, H, W);
}

int him_diffaug_fwd(const float* x, const int* table, float* y, int B, int C, int c0, int H, int W, int ch, int cw,
                    int policy, void* ws, size_t ws_bytes, void* stream) {
  return da_run<true>("diffaug_fwd", x, table, y, B, C, c0, H, W, ch, cw, policy, 0, C, ws, ws_bytes, ST);
}

int him_diffaug_bwd(const float* dout, const int* table, float* dx, int B, int C, int c0, int H, int W, int ch, int cw,
                    int policy, int g0, int gn, void* ws, size_t ws_bytes, void* stream) {
  return da_run<false>("diffaug_bwd", dout, table, dx, B, C, c0, H, W, ch, cw, policy, g0, gn, ws, ws_bytes, ST);
}

int him_diffaug_draw(int* table, int B, int H, int W, long long seed, long long step, long long sample0, int policy,
                     double ratio_translation, double ratio_cutout, int* ch, int* cw, void* stream) {
  if (!table || !ch || !cw) return fail(HIM_E_INVALID, "diffaug_draw: null pointer");
  if (B < 0 || H < 1 || W < 1) return fail(HIM_E_INVALID, "diffaug_draw: B < 0, H < 1 or W < 1");
  if (policy & ~7) return fail(HIM_E_INVALID, "diffaug_draw: unknown policy bits");
  if (!(ratio_translation >= 0.0 && ratio_translation <= 1024.0) || !(ratio_cutout >= 0.0 && ratio_cutout <= 1024.0))
    return fail(HIM_E_INVALID, "diffaug_draw: a ratio is negative, NaN or above 1024");
  if ((long long)H > (1 << 20) || (long long)W > (1 << 20)) return fail(HIM_E_INVALID, "diffaug_draw: H or W above 2^20");
  const int sy = (int)floor((double)H * ratio_translation + 0.5), sx = (int)floor((double)W * ratio_translation + 0.5);
  const bool cut = (policy & DA_CUTOUT) != 0;
  const int h = cut ? (int)floor((double)H * ratio_cutout + 0.5) : 0, w = cut ? (int)floor((double)W * ratio_cutout + 0.5) : 0;
  *ch = h;
  *cw = w;
  if (B == 0) return HIM_OK;
  hipLaunchKernelGGL(da_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ST, table, B, H, W,
                     (unsigned long long)seed, (unsigned long long)step, (unsigned long long)sample0, policy, sy, sx, h, w);
  return check_launch("diffaug_draw");
}

}  // extern "C"
