// Distance-feathered, shape-aware compositing of a joint edit (include/him.h "Feathered canvas composite"): the pixels a
// layout edit changed (him_canvas_changed -> him_edt) and the paste window's own border decide, per pixel, how much of
// the generated patch replaces the photograph.  him_canvas_paste_blend_v is him_canvas_paste_bicubic_v's column pass
// (csrc/him_data.hip: same tmp, same tables, same Pillow 8-bit fixed point) with that matte applied on the way into the
// canvas.  Memory-bound: per window pixel the tmp column taps (3 bytes each), 12 bytes of canvas in and out, 4 bytes of
// dist2 and 4 of matte; no LDS, no atomics, no workspace.
//
// Tile: a 256-thread workgroup owns CMP_TW = 64 columns x CMP_TH = 4 rows of the window, lane = column, one wave per
// row, one pixel per thread.  A wave's canvas, dist2 and matte accesses are 256 contiguous bytes per plane row, its tmp
// reads 192 contiguous bytes per tap; first / count / weights of the row are wave-uniform (scalar loads).  Tiles are
// numbered along one grid axis (row-major), so neither window side is bound by the 65535 limit of the other axes.
// Every canvas element is read and written by the one thread that owns it; nothing outside the window is touched.
//
// him_canvas_seamless_apply (include/him.h "Seamless canvas composite") writes clamp(P + m, 0, 1) -- the patch plus the
// membrane of csrc/him_membrane.hip -- into the window's interior through the same matte (cmp_alpha) on the same tile.
#include "him_common.h"

namespace him {

#define CMP_TW 64
#define CMP_TH 4
#define CMP_PRECISION_BITS 22   // DATA_PRECISION_BITS of him_data.hip (Pillow's PRECISION_BITS)
#define CMP_MAX_RADIUS 16384    // feather and reach: (reach + feather)^2 <= 2^30, next to him_edt's dx^2 + dy^2 < 2^30

__device__ __forceinline__ int cmp_clip8(int v) {
  v >>= CMP_PRECISION_BITS;  // arithmetic shift, as Pillow's clip8_lookups index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// changed[y][x] = before[y0+y][x0+x] != after[y0+y][x0+x] over one-channel fp32 id canvases (Hc, Wc)
__global__ void __launch_bounds__(CMP_TW* CMP_TH)
    canvas_changed_kernel(const float* __restrict__ before, const float* __restrict__ after, int Wc, int x0, int y0, int H,
                          int W, int tiles_x, unsigned char* __restrict__ changed) {
  const int x = (int)(blockIdx.x % tiles_x) * CMP_TW + threadIdx.x;
  const int y = (int)(blockIdx.x / tiles_x) * CMP_TH + threadIdx.y;
  if (x >= W || y >= H) return;
  const long long i = (long long)(y0 + y) * Wc + x0 + x;
  changed[(long long)y * W + x] = before[i] != after[i] ? 1 : 0;
}

// The matte of window pixel (x, y): every decision (which side counts, inside / outside the ramps) is an integer
// comparison; only a value strictly inside a ramp is computed in fp32, each operation rounded on its own.
__device__ __forceinline__ float cmp_alpha(int x, int y, int Hc, int Wc, int x0, int y0, int H, int W,
                                           const int* __restrict__ dist2, int feather, int reach, int profile) {
  int db = 0x7fffffff;  // distance to the nearest window side that has canvas behind it
  if (x0 > 0) db = min(db, x + 1);
  if ((long long)x0 + W < Wc) db = min(db, W - x);
  if (y0 > 0) db = min(db, y + 1);
  if ((long long)y0 + H < Hc) db = min(db, H - y);
  float t = 1.f;
  if (db < feather) t = __fdiv_rn((float)db, (float)feather);
  if (dist2) {
    const int d2 = dist2[(long long)y * W + x];
    const long long r2 = (long long)reach * reach, o2 = (long long)(reach + feather) * (reach + feather);
    float to;
    if (d2 == HIM_EDT_NONE) to = 0.f;
    else if ((long long)d2 <= r2) to = 1.f;
    else if ((long long)d2 >= o2) to = 0.f;
    else to = __fsub_rn(1.f, __fdiv_rn(__fsub_rn(__fsqrt_rn((float)d2), (float)reach), (float)feather));
    t = fminf(t, to);
  }
  if (profile == HIM_MATTE_SMOOTH) t = __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.f, __fmul_rn(2.f, t)));
  return t;
}

__global__ void __launch_bounds__(CMP_TW* CMP_TH)
    canvas_paste_blend_v_kernel(const unsigned char* __restrict__ tmp, const int* __restrict__ first,
                                const int* __restrict__ count, const int* __restrict__ weights, int ksize,
                                float* __restrict__ canvas, int Hc, int Wc, int x0, int y0, int H, int W,
                                const int* __restrict__ dist2, int feather, int reach, int profile,
                                float* __restrict__ matte, int tiles_x) {
  const int x = (int)(blockIdx.x % tiles_x) * CMP_TW + threadIdx.x;
  // one wave per row of the tile: the row, and with it the row's table entries, is the same in all 64 lanes
  const int y = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / tiles_x) * CMP_TH + (int)threadIdx.y);
  if (x >= W || y >= H) return;
  const float alpha = cmp_alpha(x, y, Hc, Wc, x0, y0, H, W, dist2, feather, reach, profile);
  if (matte) matte[(long long)y * W + x] = alpha;
  if (alpha == 0.f) return;  // the canvas keeps its pixel: neither the taps nor the canvas are read
  const int f = first[y], n = count[y];
  const int* w = weights + (long long)y * ksize;
  int a0 = 1 << (CMP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int k = 0; k < n; ++k) {
    const int wk = w[k];
    const unsigned char* p = tmp + ((long long)(f + k) * W + x) * 3;
    a0 += (int)p[0] * wk;
    a1 += (int)p[1] * wk;
    a2 += (int)p[2] * wk;
  }
  const int v[3] = {cmp_clip8(a0), cmp_clip8(a1), cmp_clip8(a2)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long i = ((long long)c * Hc + y0 + y) * Wc + x0 + x;
    const float P = __fdiv_rn((float)v[c], 255.f);  // what him_canvas_paste_bicubic_v writes
    if (alpha == 1.f) {
      canvas[i] = P;
    } else {
      const float O = canvas[i];
      canvas[i] = __fadd_rn(O, __fmul_rn(alpha, __fsub_rn(P, O)));
    }
  }
}

// Seamless composite (include/him.h "Seamless canvas composite"): on the window's interior the canvas takes
// v = clamp(P + m, 0, 1) through the matte of cmp_alpha (feather 0: alpha = 1); on the ring P + m is the photograph
// itself, which is written as "not written".  Same tile as canvas_paste_blend_v_kernel: lane = column, a wave per row.
__global__ void __launch_bounds__(CMP_TW* CMP_TH)
    canvas_seamless_apply_kernel(const float* __restrict__ P, const float* __restrict__ m, float* __restrict__ canvas,
                                 int Hc, int Wc, int x0, int y0, int H, int W, const int* __restrict__ dist2, int feather,
                                 int reach, int profile, float* __restrict__ matte, int tiles_x) {
  const int x = (int)(blockIdx.x % tiles_x) * CMP_TW + threadIdx.x;
  const int y = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / tiles_x) * CMP_TH + (int)threadIdx.y);
  if (x >= W || y >= H) return;
  const float alpha = feather ? cmp_alpha(x, y, Hc, Wc, x0, y0, H, W, dist2, feather, reach, profile) : 1.f;
  if (matte) matte[(long long)y * W + x] = alpha;
  if (alpha == 0.f) return;
  const int l = x0 > 0, r = (long long)x0 + W < Wc, t = y0 > 0, b = (long long)y0 + H < Hc;
  if (x < l || x >= W - r || y < t || y >= H - b) return;  // the ring keeps the photograph
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long iw = ((long long)c * H + y) * W + x;
    const long long i = ((long long)c * Hc + y0 + y) * Wc + x0 + x;
    const float v = fminf(fmaxf(__fadd_rn(P[iw], m[iw]), 0.f), 1.f);
    if (alpha == 1.f) {
      canvas[i] = v;
    } else {
      const float O = canvas[i];
      canvas[i] = __fadd_rn(O, __fmul_rn(alpha, __fsub_rn(v, O)));
    }
  }
}

// tiles of a (H, W) window along one grid axis; 0 when they do not fit it
static inline long long cmp_tiles(int H, int W, int* tiles_x) {
  *tiles_x = cdiv(W, CMP_TW);
  const long long n = (long long)*tiles_x * cdiv(H, CMP_TH);
  return n <= 0x7fffffffLL ? n : 0;
}

static inline bool cmp_window_inside(int Hc, int Wc, int x0, int y0, int H, int W) {
  return x0 >= 0 && y0 >= 0 && (long long)x0 + W <= Wc && (long long)y0 + H <= Hc;
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

int him_canvas_changed(const float* before, const float* after, int Hc, int Wc, int x0, int y0, int H, int W,
                       unsigned char* changed, void* stream) {
  if (!before || !after || !changed) return fail(HIM_E_INVALID, "canvas_changed: null pointer");
  if (H < 1 || W < 1) return fail(HIM_E_INVALID, "canvas_changed: bad shape %dx%d", W, H);
  if (!cmp_window_inside(Hc, Wc, x0, y0, H, W))
    return fail(HIM_E_INVALID, "canvas_changed: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc, Hc);
  int tiles_x;
  const long long tiles = cmp_tiles(H, W, &tiles_x);
  if (!tiles) return fail(HIM_E_INVALID, "canvas_changed: window %dx%d too large", W, H);
  hipLaunchKernelGGL(canvas_changed_kernel, dim3((unsigned)tiles), dim3(CMP_TW, CMP_TH), 0, ST, before, after, Wc, x0, y0,
                     H, W, tiles_x, changed);
  return check_launch("canvas_changed");
}

int him_canvas_paste_blend_v(const unsigned char* tmp, const int* first, const int* count, const int* weights, int ksize,
                             float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const int* dist2, int feather,
                             int reach, int profile, float* matte, void* stream) {
  if (!tmp || !first || !count || !weights || !canvas) return fail(HIM_E_INVALID, "canvas_paste_blend_v: null pointer");
  if (H < 1 || W < 1 || ksize < 1) return fail(HIM_E_INVALID, "canvas_paste_blend_v: bad shape %dx%d, ksize %d", W, H, ksize);
  if (!cmp_window_inside(Hc, Wc, x0, y0, H, W))
    return fail(HIM_E_INVALID, "canvas_paste_blend_v: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc,
                Hc);
  if (feather < 1 || feather > CMP_MAX_RADIUS)
    return fail(HIM_E_INVALID, "canvas_paste_blend_v: feather %d outside 1..%d", feather, CMP_MAX_RADIUS);
  if (reach < 0 || reach > CMP_MAX_RADIUS)
    return fail(HIM_E_INVALID, "canvas_paste_blend_v: reach %d outside 0..%d", reach, CMP_MAX_RADIUS);
  if (profile != HIM_MATTE_LINEAR && profile != HIM_MATTE_SMOOTH)
    return fail(HIM_E_INVALID, "canvas_paste_blend_v: profile %d", profile);
  int tiles_x;
  const long long tiles = cmp_tiles(H, W, &tiles_x);
  if (!tiles) return fail(HIM_E_INVALID, "canvas_paste_blend_v: window %dx%d too large", W, H);
  hipLaunchKernelGGL(canvas_paste_blend_v_kernel, dim3((unsigned)tiles), dim3(CMP_TW, CMP_TH), 0, ST, tmp, first, count,
                     weights, ksize, canvas, Hc, Wc, x0, y0, H, W, dist2, feather, reach, profile, matte, tiles_x);
  return check_launch("canvas_paste_blend_v");
}

int him_canvas_seamless_apply(const float* P, const float* m, float* canvas, int Hc, int Wc, int x0, int y0, int H, int W,
                              const int* dist2, int feather, int reach, int profile, float* matte, void* stream) {
  if (!P || !m || !canvas) return fail(HIM_E_INVALID, "canvas_seamless_apply: null pointer");
  if (H < 1 || W < 1) return fail(HIM_E_INVALID, "canvas_seamless_apply: bad shape %dx%d", W, H);
  if (!cmp_window_inside(Hc, Wc, x0, y0, H, W))
    return fail(HIM_E_INVALID, "canvas_seamless_apply: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc,
                Hc);
  if (H - (y0 > 0) - ((long long)y0 + H < Hc) < 1 || W - (x0 > 0) - ((long long)x0 + W < Wc) < 1)
    return fail(HIM_E_INVALID, "canvas_seamless_apply: a %dx%d window has no interior", W, H);
  if (feather < 0 || feather > CMP_MAX_RADIUS)
    return fail(HIM_E_INVALID, "canvas_seamless_apply: feather %d outside 0..%d", feather, CMP_MAX_RADIUS);
  if (reach < 0 || reach > CMP_MAX_RADIUS)
    return fail(HIM_E_INVALID, "canvas_seamless_apply: reach %d outside 0..%d", reach, CMP_MAX_RADIUS);
  if (feather == 0 && (dist2 || reach != 0))
    return fail(HIM_E_INVALID, "canvas_seamless_apply: dist2 and reach need a feather");
  if (profile != HIM_MATTE_LINEAR && profile != HIM_MATTE_SMOOTH)
    return fail(HIM_E_INVALID, "canvas_seamless_apply: profile %d", profile);
  int tiles_x;
  const long long tiles = cmp_tiles(H, W, &tiles_x);
  if (!tiles) return fail(HIM_E_INVALID, "canvas_seamless_apply: window %dx%d too large", W, H);
  hipLaunchKernelGGL(canvas_seamless_apply_kernel, dim3((unsigned)tiles), dim3(CMP_TW, CMP_TH), 0, ST, P, m, canvas, Hc, Wc,
                     x0, y0, H, W, dist2, feather, reach, profile, matte, tiles_x);
  return check_launch("canvas_seamless_apply");
}

}  // extern "C"
