// Feature-space set metrics (include/him.h "Feature-space set metrics"): the reduction of feature maps to descriptor
// rows, the streaming first and second moments of a descriptor matrix (Frechet distance) and the kernel sums of the
// polynomial-kernel MMD (KID).  The two arithmetic-heavy reductions run on the fp64 matrix instruction
// v_mfma_f64_16x16x4_f64 with fp32 operands widened on load: a product of two fp32 values is exact in fp64, so only the
// summation rounds.  No floating-point atomics; every sum that crosses threads goes through a fixed butterfly over the
// lanes of a wave, a fixed sum over the four waves (block_sum_f64, him_common.h), and (KID) one partial per tile in the
// workspace that a second launch adds in tile order: results are bit-identical from run to run.  The fragment layout of
// the instruction is written down in him_mfma_f64.h.
//
// him_feat_pool     a workgroup per (image, channel) plane, thread t adds elements t, t + 256, ... in double.
// him_feat_moments  a wave per 16 x 16 tile of the upper triangle of X^T X; k walks the rows four at a time; the tile is
//                   added to `second` and to its mirror image, the diagonal tile only from its own upper triangle.
// him_kid_sums      a workgroup per 64 x 64 tile of pairs, a wave per 32 x 32 (gram_tile_32x32, him_mfma_f64.h).  The
//                   cube and the masks (diagonal by position, ragged edge) run on the accumulators; the Gram matrix is
//                   never stored.  Tiles below the diagonal of the xx and yy blocks are skipped, those above count twice.
#include <math.h>

#include "him_common.h"
#include "him_mfma_f64.h"

namespace him {

#define KID_TILE 64
#define KID_MAX_M 65536

// ---- pool -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feat_pool_kernel(const float* __restrict__ x, long long planes, int C, long long hw,
                                                        float* __restrict__ feat, long long row0, int D, int c0) {
  __shared__ double sh[4];
  for (long long p = blockIdx.x; p < planes; p += gridDim.x) {
    const float* in = x + (size_t)p * hw;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < hw; i += 256) acc += (double)in[i];
    const double r = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) {
      const long long b = p / C, c = p - b * C;
      feat[(size_t)(row0 + b) * D + c0 + c] = (float)(r / (double)hw);
    }
  }
}

// ---- moments ----------------------------------------------------------------------------------------------------------
// thread j owns column j and walks the rows in order
__global__ __launch_bounds__(256) void feat_sum_kernel(const float* __restrict__ rows, long long n, int D,
                                                       double* __restrict__ sum) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  double a = 0.0;
  for (long long i = 0; i < n; ++i) a += (double)rows[(size_t)i * D + j];
  sum[j] += a;
}

// wave -> tile (ta, tb) of X^T X, ta <= tb: C[m][n] = sum_i X[i][16 ta + m] X[i][16 tb + n]
__global__ __launch_bounds__(256) void feat_second_kernel(const float* __restrict__ rows, long long n, int D, int T,
                                                          double* __restrict__ second) {
  const int lane = threadIdx.x & 63;
  const long long t = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (t >= (long long)T * T) return;                      // wave-uniform
  const int ta = (int)(t / T), tb = (int)(t - (long long)ta * T);
  if (tb < ta) return;                                    // wave-uniform
  const int r = lane >> 4, c = lane & 15;
  const int ca = ta * 16 + c, cb = tb * 16 + c;
  const bool oka = ca < D, okb = cb < D;
  mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long long i0 = 0; i0 < n; i0 += 4) {
    const long long i = i0 + r;
    double a = 0.0, b = 0.0;                              // padding lives in registers: nothing is read past a row
    if (i < n) {
      const float* row = rows + (size_t)i * D;
      if (oka) a = (double)row[ca];
      if (okb) b = (double)row[cb];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ga = ta * 16 + r + 4 * q, gb = cb;          // row (lane >> 4) + 4 q, column lane & 15
    if (ga >= D || gb >= D || (ta == tb && ga > gb)) continue;
    const size_t up = (size_t)ga * D + gb, low = (size_t)gb * D + ga;
    const double v = second[up] + acc[q];                 // both triangles hold the same bits before and after
    second[up] = v;
    if (ga != gb) second[low] = v;
  }
}

// ---- KID --------------------------------------------------------------------------------------------------------------
// the row an index of the table stands for; an index outside the matrix is replaced (and reported by the second launch)
__device__ __forceinline__ const float* kid_row(const float* __restrict__ base, long long n_rows, const int* __restrict__ idx,
                                                int pos, int m, int D) {
  long long r = pos < m ? (long long)idx[pos] : 0;
  if (r < 0 || r >= n_rows) r = 0;
  return base + (size_t)r * D;
}

// grid (T * T, 3, n_subsets); kind 0: xx, 1: yy, 2: xy.  One partial per tile: ws[(s * 3 + kind) * T * T + tile].
__global__ __launch_bounds__(256) void kid_tile_kernel(const float* __restrict__ x, long long nx, const float* __restrict__ y,
                                                       long long ny, int D, const int* __restrict__ ix,
                                                       const int* __restrict__ iy, int m, int T, double gamma, double coef0,
                                                       int vec, double* __restrict__ ws) {
  __shared__ double sh[4];
  const int kind = blockIdx.y, s = blockIdx.z;
  const int ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
  if (kind < 2 && tj < ti) return;                        // the mirror image of a tile above the diagonal
  const float* am = kind == 1 ? y : x;
  const float* bm = kind == 0 ? x : y;
  const long long na = kind == 1 ? ny : nx, nb = kind == 0 ? nx : ny;
  const int* ia = (kind == 1 ? iy : ix) + (size_t)s * m;
  const int* ib = (kind == 0 ? ix : iy) + (size_t)s * m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int i_base = ti * KID_TILE + (wave >> 1) * 32, j_base = tj * KID_TILE + (wave & 1) * 32;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    pa[u] = kid_row(am, na, ia, i_base + u * 16 + c, m, D);
    pb[u] = kid_row(bm, nb, ib, j_base + u * 16 + c, m, D);
  }
  mfma_d4 acc[2][2];
  gram_tile_32x32(pa[0], pa[1], pb[0], pb[1], D, vec, g, acc);
  double part = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i_base + u * 16 + g + 4 * q, j = j_base + v * 16 + c;   // row (lane >> 4) + 4 q, column lane & 15
        if (i < m && j < m && (kind == 2 || i != j)) {
          const double t = gamma * acc[u][v][q] + coef0;
          part += t * t * t;
        }
      }
  const double r = block_sum_f64(part, sh);
  if (threadIdx.x == 0) ws[((size_t)s * 3 + kind) * T * T + blockIdx.x] = (kind < 2 && tj > ti) ? 2.0 * r : r;
}

// a workgroup per subset: checks the subset's indices and adds its tiles in tile order
__global__ __launch_bounds__(256) void kid_reduce_kernel(const double* __restrict__ ws, const int* __restrict__ ix,
                                                         const int* __restrict__ iy, long long nx, long long ny, int m, int T,
                                                         double* __restrict__ out, int* __restrict__ status) {
  __shared__ double sh[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  int bad = 0;
  for (int i = tid; i < m; i += 256) {
    const long long a = ix[(size_t)s * m + i], b = iy[(size_t)s * m + i];
    bad |= (a < 0 || a >= nx || b < 0 || b >= ny) ? 1 : 0;
  }
  bad = __syncthreads_or(bad);
  for (int kind = 0; kind < 3; ++kind) {
    const double* part = ws + ((size_t)s * 3 + kind) * T * T;
    double acc = 0.0;
    for (int t = tid; t < T * T; t += 256) {
      const int ti = t / T, tj = t - ti * T;
      if (kind == 2 || tj >= ti) acc += part[t];
    }
    const double r = block_sum_f64(acc, sh);
    if (tid == 0) out[(size_t)s * 3 + kind] = bad ? (double)NAN : r;
  }
  if (bad && tid == 0) atomicOr(status, HIM_KID_BAD_INDEX);
}

static inline bool kid_shape_ok(int n_subsets, int m) { return n_subsets >= 1 && n_subsets <= 65535 && m >= 2 && m <= KID_MAX_M; }
static inline size_t kid_ws_bytes(int n_subsets, int m) {
  const size_t T = (size_t)(m + KID_TILE - 1) / KID_TILE;
  return (size_t)n_subsets * 3 * T * T * sizeof(double);
}
static inline bool moments_shape_ok(long long n, int D) { return n >= 1 && n <= (1LL << 40) && D >= 1 && D <= HIM_FEAT_MAX_DIM; }

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

int him_feat_pool(const float* x, int B, int C, int h, int w, float* feat, long long capacity, long long row0, int D, int c0,
                  void* stream) {
  if (B < 1 || C < 1 || h < 1 || w < 1 || (long long)h * w > 0x7FFFFFFFLL || (long long)B * C > (1LL << 40) / ((long long)h * w))
    return fail(HIM_E_INVALID, "feat_pool: bad shape (B %d, C %d, h %d, w %d; all >= 1, B C h w <= 2^40)", B, C, h, w);
  if (D < 1 || c0 < 0 || (long long)c0 + C > D)
    return fail(HIM_E_INVALID, "feat_pool: columns [%d, %lld) outside a row of %d", c0, (long long)c0 + C, D);
  if (row0 < 0 || capacity < 1 || row0 + B > capacity || capacity > (1LL << 40))
    return fail(HIM_E_INVALID, "feat_pool: rows [%lld, %lld) outside capacity %lld", row0, row0 + B, capacity);
  if (!x || !feat) return fail(HIM_E_INVALID, "feat_pool: null pointer");
  if ((uintptr_t)x % 4 != 0 || (uintptr_t)feat % 4 != 0) return fail(HIM_E_INVALID, "feat_pool: a pointer is not 4-byte aligned");
  const long long planes = (long long)B * C;
  hipLaunchKernelGGL(feat_pool_kernel, dim3((unsigned)(planes < 65535 ? planes : 65535)), dim3(256), 0, ST, x, planes, C,
                     (long long)h * w, feat, row0, D, c0);
  return check_launch("feat_pool");
}

size_t him_feat_moments_ws(long long n, int D) { return moments_shape_ok(n, D) ? 16 : 0; }

int him_feat_moments(const float* feat, long long row0, long long n, int D, double* sum, double* second, void* ws,
                     size_t ws_bytes, void* stream) {
  if (D < 1 || D > HIM_FEAT_MAX_DIM) return fail(HIM_E_INVALID, "feat_moments: D %d outside 1..%d", D, HIM_FEAT_MAX_DIM);
  if (row0 < 0 || row0 > (1LL << 40) || !moments_shape_ok(n, D))
    return fail(HIM_E_INVALID, "feat_moments: rows [%lld, %lld) (row0 >= 0, n >= 1, at most 2^40)", row0, row0 + n);
  if (!feat || !sum || !second || !ws) return fail(HIM_E_INVALID, "feat_moments: null pointer");
  if ((uintptr_t)feat % 4 != 0 || (uintptr_t)sum % 8 != 0 || (uintptr_t)second % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID, "feat_moments: a pointer is not aligned to its element size");
  if (ws_bytes < 16) return fail(HIM_E_WORKSPACE, "feat_moments: workspace %zu < %zu bytes", ws_bytes, (size_t)16);
  const float* rows = feat + (size_t)row0 * D;
  const int T = cdiv(D, 16);
  hipLaunchKernelGGL(feat_sum_kernel, dim3((unsigned)cdiv(D, 256)), dim3(256), 0, ST, rows, n, D, sum);
  hipLaunchKernelGGL(feat_second_kernel, dim3((unsigned)cdiv((long long)T * T, 4)), dim3(256), 0, ST, rows, n, D, T, second);
  return check_launch("feat_moments");
}

size_t him_kid_sums_ws(int n_subsets, int m) { return kid_shape_ok(n_subsets, m) ? kid_ws_bytes(n_subsets, m) : 0; }

int him_kid_sums(const float* x, long long nx, const float* y, long long ny, int D, const int* ix, const int* iy, int n_subsets,
                 int m, double gamma, double coef0, double* out, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (!kid_shape_ok(n_subsets, m))
    return fail(HIM_E_INVALID, "kid_sums: n_subsets %d (1..65535), m %d (2..%d)", n_subsets, m, KID_MAX_M);
  if (D < 1 || D > (1 << 20) || nx < 1 || ny < 1 || nx > 0x7FFFFFFFLL || ny > 0x7FFFFFFFLL)
    return fail(HIM_E_INVALID, "kid_sums: nx %lld, ny %lld, D %d (rows 1..2^31 - 1, D 1..2^20)", nx, ny, D);
  if (!(gamma >= 0.0) || !(gamma <= 1e300) || !(fabs(coef0) <= 1e300))
    return fail(HIM_E_INVALID, "kid_sums: gamma %g (>= 0, 0 means 1 / D), coef0 %g (finite)", gamma, coef0);
  if (!x || !y || !ix || !iy || !out || !status || !ws) return fail(HIM_E_INVALID, "kid_sums: null pointer");
  if ((uintptr_t)x % 4 != 0 || (uintptr_t)y % 4 != 0 || (uintptr_t)ix % 4 != 0 || (uintptr_t)iy % 4 != 0 ||
      (uintptr_t)status % 4 != 0 || (uintptr_t)out % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID, "kid_sums: a pointer is not aligned to its element size");
  const size_t need = kid_ws_bytes(n_subsets, m);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "kid_sums: workspace %zu < %zu bytes", ws_bytes, need);
  const int T = cdiv(m, KID_TILE);
  const int vec = gram_vec_ok(D, x, y);
  hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)(T * T), 3, (unsigned)n_subsets), dim3(256), 0, ST, x, nx, y, ny, D, ix, iy,
                     m, T, gamma == 0.0 ? 1.0 / (double)D : gamma, coef0, vec, (double*)ws);
  hipLaunchKernelGGL(kid_reduce_kernel, dim3((unsigned)n_subsets), dim3(256), 0, ST, (const double*)ws, ix, iy, nx, ny, m, T, out,
                     status);
  return check_launch("kid_sums");
}

}  // extern "C"
