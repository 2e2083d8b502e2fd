// Exact Euclidean distance transform of label planes and the boundary statistics built on it (include/him.h "Distance
// transform and boundary metrics").  Integer work throughout; the one floating-point value, the sum of distances, is
// added in a fixed order in double.
//
// him_edt, three launches:
//   status   one thread per job: seed count 0, the refused-job flag.
//   row pass one 256-thread workgroup per (row, job).  Two scans along the row, 256 columns a step with a carry: a prefix
//            maximum of "x if seed else -1" walking right (the nearest seed at or left of x, kept in LDS) and a suffix
//            minimum walking left (the nearest seed at or right of x).  The nearer of the two, the left one on a tie, goes
//            to the workspace as an int16 column index (-1: the row has no seed).  Seeds are counted with one integer
//            atomic per wave.
//   column pass  one workgroup per (tile of EDT_TW columns x EDT_TH rows, job); lane = column, every thread owns
//            EDT_RPT = EDT_TH / 4 consecutive rows of its column.  The workspace rows are staged in LDS EDT_CH at a time
//            as (x - x')^2 (2^30 where the row has no seed) and every thread minimises (x - x')^2 + (y - y')^2 over y'.
//            The chunk holding the tile goes first and the sweep walks UP in decreasing y' with <=, then DOWN from the
//            next chunk in increasing y' with <: among equal distances the smallest y' stays, and within a row the row
//            pass took the smallest x'.  A sweep ends as soon as no thread of the workgroup can still improve (the chunk's
//            row gap squared against the thread's worst current distance, voted with __syncthreads_or), so the work
//            follows the distances found, and is bounded by H.  A job without a seed is answered from its seed count.
// him_boundary_stats, two launches: one workgroup per (EDT_SROWS rows, job) writes four integers and one double to its
// own workspace slot; the second launch adds a job's slots in a fixed order.  No floating-point atomics.
#include <math.h>

#include "him_common.h"

namespace him {

#define EDT_TW 64                 // columns of a column-pass tile (one wave wide)
#define EDT_TH 32                 // output rows of a column-pass tile
#define EDT_RPT (EDT_TH / 4)      // rows per thread
#define EDT_CH 64                 // rows staged in LDS per step (a multiple of EDT_TH: a tile lies inside one chunk)
#define EDT_BIG (1 << 30)         // "no seed in this row": above every real distance (< 2^30), and EDT_BIG + dy^2 < 2^31
#define EDT_MAXDIM 16384
#define EDT_SROWS 16              // rows per workgroup of the statistics pass
#define EDT_SPART 5               // 8-byte words per statistics slot

__device__ __forceinline__ bool edt_eq(unsigned char c, int v) { return (int)c == v; }
__device__ __forceinline__ bool edt_eq(int c, int v) { return c == v; }
__device__ __forceinline__ bool edt_eq(long long c, int v) { return c == (long long)v; }
__device__ __forceinline__ bool edt_eq(float c, int v) { return c == (float)v; }

__device__ __forceinline__ bool edt_bad_job(int b, int rule, int B) {
  return b < 0 || b >= B || rule < HIM_EDT_NONZERO || rule > HIM_EDT_ANY_BOUNDARY;
}

// is (y, x) of `plane` a seed under `rule`?  Neighbours outside the plane do not exist: the border makes no boundary.
template <typename T>
__device__ __forceinline__ bool edt_seed(const T* __restrict__ plane, int H, int W, int y, int x, int v, int rule) {
  const size_t i = (size_t)y * W + x;
  const T c = plane[i];
  if (rule == HIM_EDT_NONZERO) return c != T(0);
  if (rule == HIM_EDT_EQUALS) return edt_eq(c, v);
  if (rule == HIM_EDT_BOUNDARY_OF && !edt_eq(c, v)) return false;
  bool differs = false;
  if (x > 0) differs |= plane[i - 1] != c;
  if (x + 1 < W) differs |= plane[i + 1] != c;
  if (y > 0) differs |= plane[i - W] != c;
  if (y + 1 < H) differs |= plane[i + W] != c;
  return differs;
}

__global__ void edt_status_kernel(const int* __restrict__ jobs, int B, int K, int* __restrict__ status) {
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < K; k += (long long)gridDim.x * blockDim.x) {
    status[2 * k] = 0;
    status[2 * k + 1] = edt_bad_job(jobs[3 * k], jobs[3 * k + 2], B) ? HIM_EDT_BAD_JOB : 0;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void edt_row_kernel(const T* __restrict__ src, const int* __restrict__ jobs, int B, int H,
                                                      int W, int K, short* __restrict__ g, int* __restrict__ status) {
  __shared__ short lft[EDT_MAXDIM];
  __shared__ int wred[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, y = blockIdx.x;
  const int steps = (W + 255) / 256;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const int b = jobs[3 * k], v = jobs[3 * k + 1], rule = jobs[3 * k + 2];
    short* row = g + ((size_t)k * H + y) * W;
    if (edt_bad_job(b, rule, B)) {  // uniform for the workgroup
      for (int x = tid; x < W; x += 256) row[x] = -1;
      continue;
    }
    const T* plane = src + (size_t)b * H * W;
    // walking right: the nearest seed at or left of x
    int carry = -1, cnt = 0;
    for (int s = 0; s < steps; ++s) {
      const int x = s * 256 + tid;
      const bool seed = x < W && edt_seed(plane, H, W, y, x, v, rule);
      cnt += seed ? 1 : 0;
      int m = seed ? x : -1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(m, o, 64);
        if (lane >= o) m = max(m, t);
      }
      if (lane == 63) wred[wave] = m;
      __syncthreads();
      int all = carry;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) m = max(m, wred[w]);
        all = max(all, wred[w]);
      }
      m = max(m, carry);
      carry = all;
      if (x < W) lft[x] = (short)m;
      __syncthreads();
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0 && cnt) atomicAdd(&status[2 * k], cnt);
    // walking left: the nearest seed at or right of x; every thread reads back the lft cells it wrote itself
    carry = EDT_BIG;
    for (int s = steps - 1; s >= 0; --s) {
      const int x = s * 256 + tid;
      const int l = x < W ? (int)lft[x] : -1;
      int m = (x < W && l == x) ? x : EDT_BIG;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(m, o, 64);
        if (lane + o < 64) m = min(m, t);
      }
      if (lane == 0) wred[wave] = m;
      __syncthreads();
      int all = carry;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w > wave) m = min(m, wred[w]);
        all = min(all, wred[w]);
      }
      m = min(m, carry);
      carry = all;
      if (x < W) {
        int pick;
        if (l < 0) pick = m == EDT_BIG ? -1 : m;
        else if (m == EDT_BIG) pick = l;
        else pick = (x - l <= m - x) ? l : m;  // the left seed on a tie
        row[x] = (short)pick;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void edt_col_kernel(const short* __restrict__ g, const int* __restrict__ status, int H,
                                                      int W, int K, int tiles_x, int* __restrict__ dist2,
                                                      int* __restrict__ nearest) {
  __shared__ int col[EDT_CH][EDT_TW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int tx = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int x0 = tx * EDT_TW, x = x0 + lane;
  const int t0 = tile_y * EDT_TH, y0 = t0 + (tid >> 6) * EDT_RPT;
  const bool active = x < W && y0 < H;
  const int cstar = t0 / EDT_CH, chunks = (H + EDT_CH - 1) / EDT_CH;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    int* out = dist2 + (size_t)k * H * W;
    int* near = nearest ? nearest + (size_t)k * H * W : nullptr;
    if (status[2 * k] == 0) {  // uniform: no seed, or a refused job
      if (active)
        for (int j = 0; j < EDT_RPT && y0 + j < H; ++j) {
          out[(size_t)(y0 + j) * W + x] = HIM_EDT_NONE;
          if (near) near[(size_t)(y0 + j) * W + x] = -1;
        }
      continue;
    }
    const short* gk = g + (size_t)k * H * W;
    int best[EDT_RPT], by[EDT_RPT];
#pragma unroll
    for (int j = 0; j < EDT_RPT; ++j) best[j] = (active && y0 + j < H) ? 0x7fffffff : 0, by[j] = 0;
    // up: the tile's own chunk first, then towards row 0, y' decreasing, <= (the smaller y' wins a tie)
    for (int c = cstar; c >= 0; --c) {
      const int c0 = c * EDT_CH, c1 = min(c0 + EDT_CH, H);
      int mb = 0;
#pragma unroll
      for (int j = 0; j < EDT_RPT; ++j) mb = max(mb, best[j]);
      const int gap = max(y0 - (c1 - 1), 0);
      const bool need = active && gap * gap <= mb;
      if (!__syncthreads_or(need ? 1 : 0)) break;
      for (int i = tid; i < (c1 - c0) * EDT_TW; i += 256) {
        const int r = i >> 6, xx = x0 + (i & 63);
        const int gx = xx < W ? (int)gk[(size_t)(c0 + r) * W + xx] : -1;
        col[r][i & 63] = gx < 0 ? EDT_BIG : __mul24(xx - gx, xx - gx);
      }
      __syncthreads();
      if (need)
        for (int r = c1 - c0 - 1; r >= 0; --r) {
          const int vv = col[r][lane], yy = c0 + r;
#pragma unroll
          for (int j = 0; j < EDT_RPT; ++j) {
            const int dy = y0 + j - yy, d = __mul24(dy, dy) + vv;
            if (d <= best[j]) best[j] = d, by[j] = yy;
          }
        }
    }
    // down: y' increasing, strict <
    for (int c = cstar + 1; c < chunks; ++c) {
      const int c0 = c * EDT_CH, c1 = min(c0 + EDT_CH, H);
      int mb = 0;
#pragma unroll
      for (int j = 0; j < EDT_RPT; ++j) mb = max(mb, best[j]);
      const int gap = c0 - (y0 + EDT_RPT - 1);  // > 0: the chunk lies below the tile
      const bool need = active && gap * gap < mb;
      if (!__syncthreads_or(need ? 1 : 0)) break;
      for (int i = tid; i < (c1 - c0) * EDT_TW; i += 256) {
        const int r = i >> 6, xx = x0 + (i & 63);
        const int gx = xx < W ? (int)gk[(size_t)(c0 + r) * W + xx] : -1;
        col[r][i & 63] = gx < 0 ? EDT_BIG : __mul24(xx - gx, xx - gx);
      }
      __syncthreads();
      if (need)
        for (int r = 0; r < c1 - c0; ++r) {
          const int vv = col[r][lane], yy = c0 + r;
#pragma unroll
          for (int j = 0; j < EDT_RPT; ++j) {
            const int dy = y0 + j - yy, d = __mul24(dy, dy) + vv;
            if (d < best[j]) best[j] = d, by[j] = yy;
          }
        }
    }
    if (active)
#pragma unroll
      for (int j = 0; j < EDT_RPT; ++j) {
        if (y0 + j >= H) break;
        const size_t o = (size_t)(y0 + j) * W + x;
        const bool none = best[j] >= EDT_BIG;
        out[o] = none ? HIM_EDT_NONE : best[j];
        if (near) near[o] = none ? -1 : by[j] * W + (int)gk[(size_t)by[j] * W + x];
      }
  }
}

// scores (PK 4: the channel of the maximum, the lowest on a tie) or probabilities (PK 5: p > 0.5) to int32 ids
__global__ void label_ids_kernel(const float* __restrict__ src, int pk, int C, long long hw, long long total,
                                 int* __restrict__ ids) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (pk == 5) {
      ids[i] = src[i] > 0.5f ? 1 : 0;
      continue;
    }
    const long long b = i / hw, p = i - b * hw;
    const float* s = src + (size_t)b * C * hw + p;
    float top = s[0];
    int lab = 0;
    for (int c = 1; c < C; ++c) {
      const float t = s[(size_t)c * hw];
      if (t > top) top = t, lab = c;
    }
    ids[i] = lab;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void edt_stats_kernel(const T* __restrict__ src, const int* __restrict__ jobs, int B, int H,
                                                        int W, int K, const int* __restrict__ dist2, int tol2, int parts,
                                                        long long* __restrict__ slots) {
  __shared__ long long ri[4][4];
  __shared__ double rd[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, part = blockIdx.x;
  const int r0 = part * EDT_SROWS, r1 = min(r0 + EDT_SROWS, H);
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const int b = jobs[3 * k], v = jobs[3 * k + 1], rule = jobs[3 * k + 2];
    int n = 0, hit = 0, far = -1, lost = 0;
    double sum = 0.0;
    if (!edt_bad_job(b, rule, B)) {
      const T* plane = src + (size_t)b * H * W;
      const int* dk = dist2 + (size_t)k * H * W;
      for (int y = r0; y < r1; ++y)
        for (int x = tid; x < W; x += 256) {
          if (!edt_seed(plane, H, W, y, x, v, rule)) continue;
          const int d = dk[(size_t)y * W + x];
          ++n;
          if (d == HIM_EDT_NONE) {
            ++lost;
          } else {
            hit += d <= tol2 ? 1 : 0;
            far = max(far, d);
            sum += sqrt((double)d);
          }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      n += __shfl_xor(n, o, 64);
      hit += __shfl_xor(hit, o, 64);
      lost += __shfl_xor(lost, o, 64);
      far = max(far, __shfl_xor(far, o, 64));
      sum += __shfl_xor(sum, o, 64);
    }
    if (lane == 0) ri[wave][0] = n, ri[wave][1] = hit, ri[wave][2] = far, ri[wave][3] = lost, rd[wave] = sum;
    __syncthreads();
    long long* slot = slots + ((size_t)k * parts + part) * EDT_SPART;
    if (tid < 4) slot[tid] = tid == 2 ? max(max(ri[0][2], ri[1][2]), max(ri[2][2], ri[3][2]))
                                      : (ri[0][tid] + ri[1][tid]) + (ri[2][tid] + ri[3][tid]);
    if (tid == 4) ((double*)slot)[4] = (rd[0] + rd[1]) + (rd[2] + rd[3]);
    __syncthreads();
  }
}

// one workgroup per job: thread t adds the slots t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void edt_stats_sum_kernel(const long long* __restrict__ slots, int parts, int K,
                                                            long long* __restrict__ counts, double* __restrict__ sumd) {
  __shared__ long long ri[4][256];
  __shared__ double rd[256];
  const int tid = threadIdx.x;
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    long long a[4] = {0, 0, -1, 0};
    double s = 0.0;
    for (int t = tid; t < parts; t += 256) {
      const long long* slot = slots + ((size_t)k * parts + t) * EDT_SPART;
      a[0] += slot[0], a[1] += slot[1], a[2] = max(a[2], slot[2]), a[3] += slot[3];
      s += ((const double*)slot)[4];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ri[q][tid] = a[q];
    rd[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) {
        ri[0][tid] += ri[0][tid + h], ri[1][tid] += ri[1][tid + h], ri[3][tid] += ri[3][tid + h];
        ri[2][tid] = max(ri[2][tid], ri[2][tid + h]);
        rd[tid] += rd[tid + h];
      }
      __syncthreads();
    }
    if (tid < 4) counts[(size_t)k * 4 + tid] = ri[tid][0];
    if (tid == 4) sumd[k] = rd[0];
    __syncthreads();
  }
}

static inline bool edt_shape_ok(int K, int H, int W) {
  return K >= 1 && H >= 1 && W >= 1 && H <= EDT_MAXDIM && W <= EDT_MAXDIM && (long long)K * H * W <= (1LL << 40);
}
static inline size_t edt_ws_bytes(int K, int H, int W) { return ((size_t)K * H * W * sizeof(short) + 15) / 16 * 16; }
static inline int edt_parts(int H) { return (H + EDT_SROWS - 1) / EDT_SROWS; }
static inline size_t edt_stats_ws_bytes(int K, int H) { return (size_t)K * edt_parts(H) * EDT_SPART * 8; }
static inline unsigned edt_job_grid(int K) { return (unsigned)(K < 65535 ? K : 65535); }

static const int edt_esize[4] = {1, 4, 8, 4};

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_edt_workspace(int K, int H, int W) { return edt_shape_ok(K, H, W) ? edt_ws_bytes(K, H, W) : 0; }

int him_edt(const void* src, int kind, int B, int H, int W, const int* jobs, int K, int* dist2, int* nearest, int* status,
            void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || H < 1 || W < 1 || H > EDT_MAXDIM || W > EDT_MAXDIM)
    return fail(HIM_E_INVALID, "edt: bad shape (B >= 1, 1 <= H, W <= %d)", EDT_MAXDIM);
  if (K < 1 || (long long)K * H * W > (1LL << 40)) return fail(HIM_E_INVALID, "edt: K %d (K >= 1, K * H * W <= 2^40)", K);
  if (kind < 0 || kind > 3) return fail(HIM_E_INVALID, "edt: kind %d", kind);
  if (!src || !jobs || !dist2 || !status || !ws) return fail(HIM_E_INVALID, "edt: null pointer");
  if ((uintptr_t)src % edt_esize[kind] != 0 || (uintptr_t)jobs % 4 != 0 || (uintptr_t)dist2 % 4 != 0 ||
      (uintptr_t)nearest % 4 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)ws % 2 != 0)
    return fail(HIM_E_INVALID, "edt: a pointer is not aligned to its element size");
  const size_t need = edt_ws_bytes(K, H, W);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "edt: workspace %zu < %zu bytes", ws_bytes, need);
  short* g = (short*)ws;
  hipLaunchKernelGGL(edt_status_kernel, dim3((unsigned)(K > 65536 ? 256 : (K + 255) / 256)), dim3(256), 0, ST, jobs, B, K,
                     status);
  const dim3 rows((unsigned)H, edt_job_grid(K));
  switch (kind) {
    case 0: hipLaunchKernelGGL(edt_row_kernel<unsigned char>, rows, dim3(256), 0, ST, (const unsigned char*)src, jobs, B, H, W, K, g, status); break;
    case 1: hipLaunchKernelGGL(edt_row_kernel<int>, rows, dim3(256), 0, ST, (const int*)src, jobs, B, H, W, K, g, status); break;
    case 2: hipLaunchKernelGGL(edt_row_kernel<long long>, rows, dim3(256), 0, ST, (const long long*)src, jobs, B, H, W, K, g, status); break;
    default: hipLaunchKernelGGL(edt_row_kernel<float>, rows, dim3(256), 0, ST, (const float*)src, jobs, B, H, W, K, g, status); break;
  }
  const int tiles_x = (W + EDT_TW - 1) / EDT_TW, tiles_y = (H + EDT_TH - 1) / EDT_TH;
  hipLaunchKernelGGL(edt_col_kernel, dim3((unsigned)(tiles_x * tiles_y), edt_job_grid(K)), dim3(256), 0, ST, (const short*)g,
                     (const int*)status, H, W, K, tiles_x, dist2, nearest);
  return check_launch("edt");
}

size_t him_boundary_stats_workspace(int K, int H, int W) { return edt_shape_ok(K, H, W) ? edt_stats_ws_bytes(K, H) : 0; }

int him_boundary_stats(const void* src, int kind, int B, int H, int W, const int* jobs, int K, const int* dist2, int tol2,
                       long long* counts, double* sumd, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || H < 1 || W < 1 || H > EDT_MAXDIM || W > EDT_MAXDIM)
    return fail(HIM_E_INVALID, "boundary_stats: bad shape (B >= 1, 1 <= H, W <= %d)", EDT_MAXDIM);
  if (K < 1 || (long long)K * H * W > (1LL << 40))
    return fail(HIM_E_INVALID, "boundary_stats: K %d (K >= 1, K * H * W <= 2^40)", K);
  if (kind < 0 || kind > 3) return fail(HIM_E_INVALID, "boundary_stats: kind %d", kind);
  if (tol2 < 0) return fail(HIM_E_INVALID, "boundary_stats: tol2 %d is negative", tol2);
  if (!src || !jobs || !dist2 || !counts || !sumd || !ws) return fail(HIM_E_INVALID, "boundary_stats: null pointer");
  if ((uintptr_t)src % edt_esize[kind] != 0 || (uintptr_t)jobs % 4 != 0 || (uintptr_t)dist2 % 4 != 0 ||
      (uintptr_t)counts % 8 != 0 || (uintptr_t)sumd % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID, "boundary_stats: a pointer is not aligned to its element size");
  const size_t need = edt_stats_ws_bytes(K, H);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "boundary_stats: workspace %zu < %zu bytes", ws_bytes, need);
  const int parts = edt_parts(H);
  const dim3 grid((unsigned)parts, edt_job_grid(K));
  long long* slots = (long long*)ws;
  switch (kind) {
    case 0: hipLaunchKernelGGL(edt_stats_kernel<unsigned char>, grid, dim3(256), 0, ST, (const unsigned char*)src, jobs, B, H, W, K, dist2, tol2, parts, slots); break;
    case 1: hipLaunchKernelGGL(edt_stats_kernel<int>, grid, dim3(256), 0, ST, (const int*)src, jobs, B, H, W, K, dist2, tol2, parts, slots); break;
    case 2: hipLaunchKernelGGL(edt_stats_kernel<long long>, grid, dim3(256), 0, ST, (const long long*)src, jobs, B, H, W, K, dist2, tol2, parts, slots); break;
    default: hipLaunchKernelGGL(edt_stats_kernel<float>, grid, dim3(256), 0, ST, (const float*)src, jobs, B, H, W, K, dist2, tol2, parts, slots); break;
  }
  hipLaunchKernelGGL(edt_stats_sum_kernel, dim3(edt_job_grid(K)), dim3(256), 0, ST, (const long long*)slots, parts, K, counts,
                     sumd);
  return check_launch("boundary_stats");
}

int him_label_ids(const float* src, int pred_kind, int B, int C, int H, int W, int* ids, void* stream) {
  if (B < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL || (long long)B * H * W > (1LL << 40))
    return fail(HIM_E_INVALID, "label_ids: bad shape");
  if (pred_kind != 4 && pred_kind != 5) return fail(HIM_E_INVALID, "label_ids: pred_kind %d (4 scores, 5 probabilities)", pred_kind);
  if (pred_kind == 4 ? C < 1 : C != 1) return fail(HIM_E_INVALID, "label_ids: C %d for pred_kind %d", C, pred_kind);
  if (!src || !ids) return fail(HIM_E_INVALID, "label_ids: null pointer");
  if ((uintptr_t)src % 4 != 0 || (uintptr_t)ids % 4 != 0) return fail(HIM_E_INVALID, "label_ids: a pointer is not 4-byte aligned");
  const long long hw = (long long)H * W, total = hw * B;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(label_ids_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, ST, src, pred_kind, C, hw,
                     total, ids);
  return check_launch("label_ids");
}

}  // extern "C"
