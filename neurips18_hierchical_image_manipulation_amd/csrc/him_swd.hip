// Sliced Wasserstein distance on Laplacian-pyramid patches (include/him.h "Set-level metrics"): the pyramid, the patch
// gather with its channel statistics, the projection onto the direction table, a segmented key sort and the distance.
// Every floating-point sum that crosses threads is added in a fixed order (a tree over thread slots, then a sequential
// walk over per-image or per-direction partials); the only atomics are integer counters and flag bits.
//
// him_lap_pyramid   down: a 256-thread workgroup per tile of 8 x 64 outputs stages the 19 x 131 inputs it needs in LDS
//                   (mirror indices resolved while staging) and filters from there; up-and-subtract: a workgroup per
//                   8 x 64 tile of level i stages the 6 x 34 cells of G_{i+1} it needs and evaluates the zero-insertion
//                   filter literally (a tap counts when its mirrored position is even in both directions).
// him_swd_gather    a workgroup per image copies the patches and reduces sum, sum of squares, minimum and maximum per
//                   channel in double to its workspace slot; a second launch walks the slots in image order.
// him_swd_project   plain FMA in double (K = 49 C <= 147 is far too short for a matrix-core pipeline to pay for its
//                   operand shuffles): tiles of 64 rows x 64 directions, one channel (49 columns) staged per step.
// him_sort_segments bitonic network on sign-fixed keys in LDS for chunks of up to HIM_SORT_LDS_MAX keys; longer segments
//                   merge the sorted chunks pairwise through global memory, every key finding its slot by a binary
//                   search of the partner run (lower bound from the left run, upper bound from the right one).
// him_swd_distance  a workgroup per direction, then one workgroup for the mean.
#include <math.h>

#include "him_common.h"

namespace him {

#define LAP_TH 8
#define LAP_TW 64
#define LAP_IN_H (2 * LAP_TH + 3)
#define LAP_IN_W (2 * LAP_TW + 3)
#define LAP_UP_H (LAP_TH / 2 + 2)
#define LAP_UP_W (LAP_TW / 2 + 2)
#define SWD_P HIM_SWD_PATCH
#define SWD_PP (SWD_P * SWD_P)
#define SWD_NSTAT 4  // sum, sum of squares, minimum, maximum

// mirror without repeating the edge (d c b | a b c d | c b a), any i
__device__ __forceinline__ int lap_mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

static inline int lap_max_levels(int H, int W) {
  const int m = H < W ? H : W;
  int l = 0;
  while (l < HIM_LAP_MAX_LEVELS && (m >> l) >= 16) ++l;
  return l;
}
static inline bool lap_shape_ok(int B, int C, int H, int W, int levels) {
  if (B < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || levels < 1 || levels > lap_max_levels(H, W)) return false;
  const int m = (1 << (levels - 1)) - 1;
  return (H & m) == 0 && (W & m) == 0 && (long long)B * C * H * W <= (1LL << 40);
}
static inline long long lap_offset(int B, int C, int H, int W, int level) {
  long long o = 0;
  for (int l = 0; l < level; ++l) o += (long long)B * C * (H >> l) * (W >> l);
  return o;
}
static inline size_t lap_ws_bytes(int B, int C, int H, int W, int levels) {
  const size_t n = (size_t)(lap_offset(B, C, H, W, levels) - lap_offset(B, C, H, W, 1)) * sizeof(float);
  return n < 16 ? 16 : (n + 15) / 16 * 16;
}

// G_{l+1} = down(G_l): src planes of h x w, dst planes of h/2 x w/2
__global__ __launch_bounds__(256) void lap_down_kernel(const float* __restrict__ src, int planes, int h, int w, int tiles_x,
                                                       float* __restrict__ dst, float* __restrict__ dst2) {
  __shared__ float tile[LAP_IN_H][LAP_IN_W + 1];
  const int tid = threadIdx.x, oh = h >> 1, ow = w >> 1;
  const int oy0 = (blockIdx.x / tiles_x) * LAP_TH, ox0 = (blockIdx.x % tiles_x) * LAP_TW;
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const float* in = src + (size_t)p * h * w;
    for (int i = tid; i < LAP_IN_H * LAP_IN_W; i += 256) {
      const int r = i / LAP_IN_W, c = i - r * LAP_IN_W;
      tile[r][c] = in[(size_t)lap_mirror(2 * oy0 - 2 + r, h) * w + lap_mirror(2 * ox0 - 2 + c, w)];
    }
    __syncthreads();
    const int lx = tid & 63, ox = ox0 + lx;
    for (int ly = tid >> 6; ly < LAP_TH; ly += 4) {
      const int oy = oy0 + ly;
      if (oy >= oh || ox >= ow) continue;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const float* row = &tile[2 * ly + i][2 * lx];
        const float hsum = (k[0] * row[0] + k[4] * row[4]) + (k[1] * row[1] + k[3] * row[3]) + k[2] * row[2];
        acc += k[i] * hsum;
      }
      const size_t o = ((size_t)p * oh + oy) * ow + ox;
      dst[o] = acc;
      if (dst2) dst2[o] = acc;
    }
    __syncthreads();
  }
}

// lap = fine - up(coarse): fine planes of h x w, coarse planes of h/2 x w/2
__global__ __launch_bounds__(256) void lap_up_sub_kernel(const float* __restrict__ fine, const float* __restrict__ coarse,
                                                         int planes, int h, int w, int tiles_x, float* __restrict__ lap) {
  __shared__ float tile[LAP_UP_H][LAP_UP_W + 1];
  const int tid = threadIdx.x, ch = h >> 1, cw = w >> 1;
  const int y0 = (blockIdx.x / tiles_x) * LAP_TH, x0 = (blockIdx.x % tiles_x) * LAP_TW;
  const int r0 = y0 / 2 - 1, c0 = x0 / 2 - 1;
  const float k2[5] = {0.125f, 0.5f, 0.75f, 0.5f, 0.125f};
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const float* g = coarse + (size_t)p * ch * cw;
    for (int i = tid; i < LAP_UP_H * LAP_UP_W; i += 256) {
      const int r = i / LAP_UP_W, c = i - r * LAP_UP_W;
      const int sy = min(max(r0 + r, 0), ch - 1), sx = min(max(c0 + c, 0), cw - 1);  // cells outside are never used
      tile[r][c] = g[(size_t)sy * cw + sx];
    }
    __syncthreads();
    const int lx = tid & 63, x = x0 + lx;
    for (int ly = tid >> 6; ly < LAP_TH; ly += 4) {
      const int y = y0 + ly;
      if (y >= h || x >= w) continue;
      float acc = 0.f;
      for (int i = 0; i < 5; ++i) {
        const int Y = lap_mirror(y + i - 2, h);
        if (Y & 1) continue;
        float hsum = 0.f;
        for (int j = 0; j < 5; ++j) {
          const int X = lap_mirror(x + j - 2, w);
          if (X & 1) continue;
          hsum += k2[j] * tile[(Y >> 1) - r0][(X >> 1) - c0];
        }
        acc += k2[i] * hsum;
      }
      const size_t o = ((size_t)p * h + y) * w + x;
      lap[o] = fine[o] - acc;
    }
    __syncthreads();
  }
}

__global__ void lap_copy_kernel(const float* __restrict__ src, long long n, float* __restrict__ dst) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

// ---- gather -----------------------------------------------------------------------------------------------------------
// fixed tree over the 256 thread slots; the result is valid in thread 0
template <int OP>
__device__ __forceinline__ double swd_block_reduce(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = OP == 0 ? sh[tid] + sh[tid + s] : (OP == 1 ? fmin(sh[tid], sh[tid + s]) : fmax(sh[tid], sh[tid + s]));
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void swd_gather_kernel(const float* __restrict__ level, int B, int C, int h, int w,
                                                         const int* __restrict__ pos, int n_patches, float* __restrict__ desc,
                                                         long long row0, double* __restrict__ slots, int* __restrict__ status) {
  __shared__ double sh[256];
  __shared__ int shc[4];
  const int tid = threadIdx.x, K = SWD_PP * C, total = n_patches * K;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    double s[3] = {0, 0, 0}, q[3] = {0, 0, 0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int clamped = 0;
    for (int e = tid; e < total; e += 256) {
      const int p = e / K, kk = e - p * K, c = kk / SWD_PP, rq = kk - c * SWD_PP, r = rq / SWD_P, qx = rq - r * SWD_P;
      const int py = pos[((size_t)b * n_patches + p) * 2], px = pos[((size_t)b * n_patches + p) * 2 + 1];
      const int y0 = min(max(py, 0), h - SWD_P), x0 = min(max(px, 0), w - SWD_P);
      if (kk == 0 && (y0 != py || x0 != px)) ++clamped;
      const float v = level[(((size_t)b * C + c) * h + y0 + r) * w + x0 + qx];
      desc[((size_t)row0 + (size_t)b * n_patches + p) * K + kk] = v;
      const double d = (double)v;
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        if (cc == c) s[cc] += d, q[cc] += d * d, mn[cc] = fmin(mn[cc], d), mx[cc] = fmax(mx[cc], d);
    }
    double* slot = slots + (size_t)b * SWD_NSTAT * C;
    for (int c = 0; c < C; ++c) {
      const double rs = swd_block_reduce<0>(s[c], sh), rq = swd_block_reduce<0>(q[c], sh);
      const double rn = swd_block_reduce<1>(mn[c], sh), rx = swd_block_reduce<2>(mx[c], sh);
      if (tid == 0) slot[c * SWD_NSTAT] = rs, slot[c * SWD_NSTAT + 1] = rq, slot[c * SWD_NSTAT + 2] = rn, slot[c * SWD_NSTAT + 3] = rx;
    }
    const int n = block_sum_i32(clamped, shc);
    if (tid == 0 && n) atomicAdd(status, n);
  }
}

// thread j owns accumulator j and adds the images' partials in image order: the result does not depend on how a set
// was cut into calls
__global__ void swd_stats_walk_kernel(const double* __restrict__ slots, int B, int C, double* __restrict__ stats) {
  const int j = threadIdx.x;
  if (j >= SWD_NSTAT * C) return;
  const int kind = j % SWD_NSTAT;
  double a = stats[j];
  for (int b = 0; b < B; ++b) {
    const double v = slots[(size_t)b * SWD_NSTAT * C + j];
    a = kind < 2 ? a + v : (kind == 2 ? fmin(a, v) : fmax(a, v));
  }
  stats[j] = a;
}

// ---- projection -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, long long N, int C,
                                                          const double* __restrict__ stats, const float* __restrict__ dirs,
                                                          int n_dirs, float* __restrict__ out, int* __restrict__ status) {
  __shared__ float xs[64][SWD_PP];
  __shared__ float ds[SWD_PP][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = SWD_PP * C;
  const long long n0 = (long long)blockIdx.x * 64;
  const int d0 = blockIdx.y * 64;
  const double count = (double)N * SWD_PP;
  double mean[3], rstd[3];
  bool flat = false;
  for (int c = 0; c < C; ++c) {
    const double m = stats[c * SWD_NSTAT] / count, var = stats[c * SWD_NSTAT + 1] / count - m * m;
    flat |= !(stats[c * SWD_NSTAT + 2] < stats[c * SWD_NSTAT + 3]) || !(var > 0.0);
    mean[c] = m, rstd[c] = 1.0 / sqrt(var);
  }
  if (flat && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) atomicOr(status, HIM_SWD_ZERO_DEVIATION);
  double acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.0;
  for (int c = 0; c < C; ++c) {
    for (int i = tid; i < 64 * SWD_PP; i += 256) {
      const int r = i / SWD_PP, k = i - r * SWD_PP;
      xs[r][k] = n0 + r < N ? desc[(size_t)(n0 + r) * K + c * SWD_PP + k] : 0.f;
    }
    for (int i = tid; i < SWD_PP * 64; i += 256) {
      const int k = i >> 6, dd = i & 63;
      ds[k][dd] = d0 + dd < n_dirs ? dirs[(size_t)(c * SWD_PP + k) * n_dirs + d0 + dd] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < SWD_PP; ++k) {
      const double z = ((double)xs[lane][k] - mean[c]) * rstd[c];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] += (double)ds[k][wave * 16 + j] * z;
    }
    __syncthreads();
  }
  if (n0 + lane < N)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int d = d0 + wave * 16 + j;
      if (d < n_dirs) out[(size_t)d * N + n0 + lane] = flat ? NAN : (float)acc[j];
    }
}

// ---- sort -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned sort_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned sort_unkey(unsigned key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// block -> chunk `ch` of segment `seg`: keys [ch * HIM_SORT_LDS_MAX, ...) of the segment, sorted in LDS, src -> dst
__global__ __launch_bounds__(256) void sort_chunks_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst,
                                                          long long N, long long chunks, int* __restrict__ status) {
  __shared__ unsigned s[HIM_SORT_LDS_MAX];
  __shared__ int shc[4];
  const int tid = threadIdx.x;
  const long long seg = blockIdx.x / chunks, ch = blockIdx.x - seg * chunks;
  const long long start = ch * HIM_SORT_LDS_MAX;
  const int len = (int)(N - start < HIM_SORT_LDS_MAX ? N - start : HIM_SORT_LDS_MAX);
  const unsigned* in = src + seg * N + start;
  unsigned* out = dst + seg * N + start;
  int P = 1;
  while (P < len) P <<= 1;
  int nans = 0;
  for (int i = tid; i < P; i += 256) {
    unsigned key = 0xFFFFFFFFu;
    if (i < len) {
      const unsigned bits = in[i];
      nans += (bits & 0x7FFFFFFFu) > 0x7F800000u ? 1 : 0;
      key = sort_key(bits);
    }
    s[i] = key;
  }
  nans = wave_sum_i32(nans);
  if ((tid & 63) == 0) shc[tid >> 6] = nans;
  __syncthreads();
  if (tid == 0) {
    const int n = (shc[0] + shc[1]) + (shc[2] + shc[3]);
    if (n) atomicAdd(status, n);
  }
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned a = s[i], b = s[p];
        if ((a > b) == ((i & k) == 0)) s[i] = b, s[p] = a;
      }
      __syncthreads();
    }
  for (int i = tid; i < len; i += 256) out[i] = sort_unkey(s[i]);
}

__global__ void sort_zero_status_kernel(int* status) { status[0] = 0; }

// one pass over runs of R keys: the runs 2p and 2p + 1 of every segment become one run of 2R in dst
__global__ __launch_bounds__(256) void sort_merge_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst,
                                                         long long total, long long N, long long R) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const long long seg = idx / N, i = idx - seg * N;
    const long long a0 = i / (2 * R) * (2 * R);
    const long long a1 = a0 + R < N ? a0 + R : N, b1 = a0 + 2 * R < N ? a0 + 2 * R : N;
    const unsigned* base = src + seg * N;
    const unsigned bits = base[i], key = sort_key(bits);
    long long lo, hi, pos;
    if (i < a1) {  // a key of the left run: behind the keys of the right run that are smaller
      lo = a1, hi = b1;
      while (lo < hi) {
        const long long m = lo + ((hi - lo) >> 1);
        if (sort_key(base[m]) < key) lo = m + 1; else hi = m;
      }
      pos = (i - a0) + (lo - a1);
    } else {  // a key of the right run: behind the keys of the left run that are smaller or equal
      lo = a0, hi = a1;
      while (lo < hi) {
        const long long m = lo + ((hi - lo) >> 1);
        if (sort_key(base[m]) <= key) lo = m + 1; else hi = m;
      }
      pos = (i - a1) + (lo - a0);
    }
    dst[seg * N + a0 + pos] = bits;
  }
}

static inline bool sort_shape_ok(long long S, long long N) {
  return S >= 1 && N >= 1 && S <= 0x7FFFFFFFLL && N <= 0x7FFFFFFFLL && S * N <= 0x7FFFFFFFLL;
}
static inline size_t sort_ws_bytes(long long S, long long N) {
  return N <= HIM_SORT_LDS_MAX ? 16 : ((size_t)S * N * sizeof(float) + 15) / 16 * 16;
}

// ---- distance ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_dir_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, int n_dirs,
                                                           long long N, double* __restrict__ dir_sums) {
  __shared__ double sh[256];
  for (int d = blockIdx.x; d < n_dirs; d += gridDim.x) {
    const float* pa = a + (size_t)d * N;
    const float* pb = b + (size_t)d * N;
    double acc = 0.0;
    for (long long n = threadIdx.x; n < N; n += 256) acc += fabs((double)pa[n] - (double)pb[n]);
    const double r = swd_block_reduce<0>(acc, sh);
    if (threadIdx.x == 0) dir_sums[d] = r;
  }
}

__global__ __launch_bounds__(256) void swd_mean_kernel(const double* __restrict__ dir_sums, int n_dirs, long long N,
                                                       double* __restrict__ mean) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int d = threadIdx.x; d < n_dirs; d += 256) acc += dir_sums[d];
  const double r = swd_block_reduce<0>(acc, sh);
  if (threadIdx.x == 0) mean[0] = r / ((double)n_dirs * (double)N);
}

static inline unsigned plane_grid(long long planes) { return (unsigned)(planes < 65535 ? planes : 65535); }

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

unsigned him_lap_levels(int H, int W, int want) {
  const int most = (H < 1 || W < 1) ? 0 : lap_max_levels(H, W);
  return want > 0 && want < most ? want : most;
}

long long him_lap_level_offset(int B, int C, int H, int W, int level) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || level < 0 || level > HIM_LAP_MAX_LEVELS) return -1;
  return lap_offset(B, C, H, W, level);
}

size_t him_lap_pyramid_ws(int B, int C, int H, int W, int levels) {
  return lap_shape_ok(B, C, H, W, levels) ? lap_ws_bytes(B, C, H, W, levels) : 0;
}

int him_lap_pyramid(const float* x, int B, int C, int H, int W, int levels, float* lap, float* gauss, void* ws,
                    size_t ws_bytes, void* stream) {
  if (B < 1 || H < 1 || W < 1 || (long long)B * 3 * H * W > (1LL << 40)) return fail(HIM_E_INVALID, "lap_pyramid: bad shape");
  if (C != 1 && C != 3) return fail(HIM_E_INVALID, "lap_pyramid: C %d (1 or 3)", C);
  if (levels < 1 || levels > lap_max_levels(H, W))
    return fail(HIM_E_INVALID, "lap_pyramid: levels %d outside 1..%d (the smallest level keeps min(H, W) >= 16)", levels,
                lap_max_levels(H, W));
  if (!lap_shape_ok(B, C, H, W, levels))
    return fail(HIM_E_INVALID, "lap_pyramid: H %d, W %d are not divisible by 2^(levels - 1) = %d", H, W, 1 << (levels - 1));
  if (!x || !lap || !ws) return fail(HIM_E_INVALID, "lap_pyramid: null pointer");
  if ((uintptr_t)x % 4 != 0 || (uintptr_t)lap % 4 != 0 || (uintptr_t)gauss % 4 != 0 || (uintptr_t)ws % 4 != 0)
    return fail(HIM_E_INVALID, "lap_pyramid: a pointer is not 4-byte aligned");
  const size_t need = lap_ws_bytes(B, C, H, W, levels);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "lap_pyramid: workspace %zu < %zu bytes", ws_bytes, need);
  const long long planes = (long long)B * C, off1 = lap_offset(B, C, H, W, 1);
  float* g = (float*)ws;  // Gaussian levels 1 .. levels - 1, packed
  for (int l = 0; l + 1 < levels; ++l) {
    const int h = H >> l, w = W >> l;
    const float* src = l == 0 ? x : g + (lap_offset(B, C, H, W, l) - off1);
    const long long o = lap_offset(B, C, H, W, l + 1) - off1;
    const int tx = cdiv(w >> 1, LAP_TW), ty = cdiv(h >> 1, LAP_TH);
    hipLaunchKernelGGL(lap_down_kernel, dim3((unsigned)(tx * ty), plane_grid(planes)), dim3(256), 0, ST, src, (int)planes, h, w,
                       tx, g + o, gauss ? gauss + o : nullptr);
  }
  for (int l = 0; l + 1 < levels; ++l) {
    const int h = H >> l, w = W >> l;
    const float* fine = l == 0 ? x : g + (lap_offset(B, C, H, W, l) - off1);
    const float* coarse = g + (lap_offset(B, C, H, W, l + 1) - off1);
    const int tx = cdiv(w, LAP_TW), ty = cdiv(h, LAP_TH);
    hipLaunchKernelGGL(lap_up_sub_kernel, dim3((unsigned)(tx * ty), plane_grid(planes)), dim3(256), 0, ST, fine, coarse,
                       (int)planes, h, w, tx, lap + lap_offset(B, C, H, W, l));
  }
  const int last = levels - 1;
  const long long n = planes * (H >> last) * (W >> last);
  const float* top = last == 0 ? x : g + (lap_offset(B, C, H, W, last) - off1);
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(lap_copy_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, ST, top, n,
                     lap + lap_offset(B, C, H, W, last));
  return check_launch("lap_pyramid");
}

size_t him_swd_gather_ws(int B, int C) {
  return (B < 1 || (C != 1 && C != 3)) ? 0 : (size_t)B * SWD_NSTAT * C * sizeof(double);
}

int him_swd_gather(const float* level, int B, int C, int h, int w, const int* pos, int n_patches, float* desc,
                   long long capacity, long long row0, double* stats, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (C != 1 && C != 3) return fail(HIM_E_INVALID, "swd_gather: C %d (1 or 3)", C);
  if (B < 1 || h < SWD_P || w < SWD_P || (long long)B * C * h * w > (1LL << 40))
    return fail(HIM_E_INVALID, "swd_gather: bad shape (B >= 1, h and w >= %d)", SWD_P);
  if (n_patches < 1 || n_patches > 65536) return fail(HIM_E_INVALID, "swd_gather: n_patches %d outside 1..65536", n_patches);
  if (row0 < 0 || capacity < 1 || row0 + (long long)B * n_patches > capacity || capacity > (1LL << 40))
    return fail(HIM_E_INVALID, "swd_gather: rows [%lld, %lld) outside capacity %lld", row0, row0 + (long long)B * n_patches,
                capacity);
  if (!level || !pos || !desc || !stats || !status || !ws) return fail(HIM_E_INVALID, "swd_gather: null pointer");
  if ((uintptr_t)level % 4 != 0 || (uintptr_t)pos % 4 != 0 || (uintptr_t)desc % 4 != 0 || (uintptr_t)status % 4 != 0 ||
      (uintptr_t)stats % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID, "swd_gather: a pointer is not aligned to its element size");
  const size_t need = (size_t)B * SWD_NSTAT * C * sizeof(double);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "swd_gather: workspace %zu < %zu bytes", ws_bytes, need);
  hipLaunchKernelGGL(swd_gather_kernel, dim3(plane_grid(B)), dim3(256), 0, ST, level, B, C, h, w, pos, n_patches, desc, row0,
                     (double*)ws, status);
  hipLaunchKernelGGL(swd_stats_walk_kernel, dim3(1), dim3(64), 0, ST, (const double*)ws, B, C, stats);
  return check_launch("swd_gather");
}

int him_swd_project(const float* desc, long long N, int C, const double* stats, const float* dirs, int n_dirs, float* out,
                    int* status, void* stream) {
  if (C != 1 && C != 3) return fail(HIM_E_INVALID, "swd_project: C %d (1 or 3)", C);
  if (N < 1 || n_dirs < 1 || n_dirs > (1 << 20) || N * n_dirs > 0x7FFFFFFFLL)
    return fail(HIM_E_INVALID, "swd_project: N %lld, n_dirs %d (both >= 1, N * n_dirs <= 2^31 - 1)", N, n_dirs);
  if (!desc || !stats || !dirs || !out || !status) return fail(HIM_E_INVALID, "swd_project: null pointer");
  if ((uintptr_t)desc % 4 != 0 || (uintptr_t)dirs % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)status % 4 != 0 ||
      (uintptr_t)stats % 8 != 0)
    return fail(HIM_E_INVALID, "swd_project: a pointer is not aligned to its element size");
  hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((n_dirs + 63) / 64)), dim3(256), 0, ST, desc,
                     N, C, stats, dirs, n_dirs, out, status);
  return check_launch("swd_project");
}

size_t him_sort_segments_ws(long long S, long long N) { return sort_shape_ok(S, N) ? sort_ws_bytes(S, N) : 0; }

int him_sort_segments(float* keys, long long S, long long N, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (!sort_shape_ok(S, N)) return fail(HIM_E_INVALID, "sort_segments: S %lld, N %lld (both >= 1, S * N <= 2^31 - 1)", S, N);
  if (!keys || !status || !ws) return fail(HIM_E_INVALID, "sort_segments: null pointer");
  if ((uintptr_t)keys % 4 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)ws % 4 != 0)
    return fail(HIM_E_INVALID, "sort_segments: a pointer is not 4-byte aligned");
  const size_t need = sort_ws_bytes(S, N);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "sort_segments: workspace %zu < %zu bytes", ws_bytes, need);
  const long long chunks = (N + HIM_SORT_LDS_MAX - 1) / HIM_SORT_LDS_MAX;
  int passes = 0;
  while ((1LL << passes) < chunks) ++passes;
  unsigned* buf[2] = {(unsigned*)keys, (unsigned*)ws};
  int cur = passes & 1;  // the last pass lands in keys
  hipLaunchKernelGGL(sort_zero_status_kernel, dim3(1), dim3(1), 0, ST, status);
  hipLaunchKernelGGL(sort_chunks_kernel, dim3((unsigned)(S * chunks)), dim3(256), 0, ST, (const unsigned*)keys, buf[cur], N, chunks,
                     status);
  const long long total = S * N, blocks = (total + 255) / 256;
  long long R = HIM_SORT_LDS_MAX;
  for (int p = 0; p < passes; ++p, R <<= 1, cur ^= 1)
    hipLaunchKernelGGL(sort_merge_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, ST,
                       (const unsigned*)buf[cur], buf[cur ^ 1], total, N, R);
  return check_launch("sort_segments");
}

int him_swd_distance(const float* a, long long Na, const float* b, long long Nb, int n_dirs, double* dir_sums, double* mean,
                     void* stream) {
  if (Na != Nb) return fail(HIM_E_INVALID, "swd_distance: the sets hold %lld and %lld rows", Na, Nb);
  if (Na < 1 || n_dirs < 1 || Na * n_dirs > 0x7FFFFFFFLL)
    return fail(HIM_E_INVALID, "swd_distance: N %lld, n_dirs %d (both >= 1, N * n_dirs <= 2^31 - 1)", Na, n_dirs);
  if (!a || !b || !dir_sums || !mean) return fail(HIM_E_INVALID, "swd_distance: null pointer");
  if ((uintptr_t)a % 4 != 0 || (uintptr_t)b % 4 != 0 || (uintptr_t)dir_sums % 8 != 0 || (uintptr_t)mean % 8 != 0)
    return fail(HIM_E_INVALID, "swd_distance: a pointer is not aligned to its element size");
  hipLaunchKernelGGL(swd_dir_sums_kernel, dim3(plane_grid(n_dirs)), dim3(256), 0, ST, a, b, n_dirs, Na, dir_sums);
  hipLaunchKernelGGL(swd_mean_kernel, dim3(1), dim3(256), 0, ST, (const double*)dir_sums, n_dirs, Na, mean);
  return check_launch("swd_distance");
}

}  // extern "C"
