// k-nearest-neighbour manifold estimates (include/him.h "Feature-space set metrics", him_knn_radii and
// him_knn_membership): the all-pairs squared distances of descriptor rows in Gram form |a|^2 + |b|^2 - 2 a.b, the k-th
// smallest per row, and the membership counts against per-row radii -- what improved precision / recall (Kynkaanniemi et
// al. 2019) and density / coverage (Naeem et al. 2020) are made of.  The dot products run on v_mfma_f64_16x16x4_f64 with
// fp32 operands widened on load (exact products; the tile and the fragment layout note are in him_mfma_f64.h: C/D register
// q of a lane holds row (lane >> 4) + 4 q, column lane & 15); the n x n matrix is never stored.  No floating-point
// atomics: the selection keeps VALUES, and the k smallest values of a multiset do not depend on the order they arrive in;
// the counts are integers.  Results are bit-identical from run to run.
//
// knn_norm_kernel     a wave per row: |x|^2 in double (exact squares, lanes stride the columns, fixed butterfly).  A row
//                     with a non-finite feature gets the norm NaN and sets HIM_KNN_NONFINITE: every distance to it is
//                     then NaN, and NaN passes neither the `<` of the selection nor the `<=` of the membership test.
//                     The same launch clears the count the row owns (membership).
// knn_radii_kernel    a workgroup per (block of 64 rows, chunk of column tiles); per 64 x 64 tile a wave computes 32 x 32
//                     (gram_tile_32x32, as in him_kid_sums), the distances go to LDS (row stride 68 doubles),
//                     and thread t -- row t >> 2, columns (t & 3) + 4 s -- pushes its 16 values through a sorted list of
//                     the KL smallest kept in registers (KL = 4, 8 or 16 >= k; compare-exchange chain, static indices).
//                     With that stride and interleave the 32 lanes of an LDS read group hit 32 different 8-byte slots.
//                     At the end of the chunk the four lists of a row are merged through LDS and the first k values go
//                     to the workspace: part[(row * n_chunks + chunk) * k + t].
// knn_merge_kernel    a thread per row merges its partial lists in chunk order and writes the k-th value.
// knn_member_kernel   a workgroup per (block of 64 query rows, every KNN_MEMBER_SPLIT-th reference tile); the indicator
//                     d2 <= radii2[reference] is summed along rows (kept in registers across the tiles) and columns by
//                     shuffles, and the non-zero sums are added with integer atomics.
#include <math.h>

#include "him_common.h"
#include "him_mfma_f64.h"

namespace him {

#define KNN_TILE 64
#define KNN_LDS_STRIDE 68          // doubles per LDS row of the distance tile
#define KNN_CHUNK_TILES 8          // column tiles per chunk (512 columns) while that gives at most KNN_MAX_CHUNKS chunks
#define KNN_MAX_CHUNKS 16          // beyond, the chunks grow: the workspace stays at n * 16 * k doubles
#define KNN_MEMBER_SPLIT 64        // reference tiles are dealt to at most this many workgroups per query block

// ---- norms ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_norm_kernel(const float* __restrict__ x, int n, int D, double* __restrict__ norm,
                                                       int* __restrict__ clear, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                     // wave-uniform
  const float* row = x + (size_t)i * D;
  double acc = 0.0;
  int bad = 0;
  for (int k = lane; k < D; k += 64) {
    const float v = row[k];
    bad |= (v - v == 0.f) ? 0 : 1;                        // inf - inf and NaN - NaN are NaN
    acc += (double)v * (double)v;
  }
  acc = wave_sum_f64(acc);
  bad = __any(bad);
  if (lane == 0) {
    norm[i] = bad ? (double)NAN : acc;
    if (clear) clear[i] = 0;
    if (bad) atomicOr(status, HIM_KNN_NONFINITE);
  }
}

// ---- the 64 x 64 Gram tile: rows by position ---------------------------------------------------------------------------
// a position outside the matrix reads row 0 (and is masked by the caller): nothing is read past the last row
__device__ __forceinline__ const float* knn_row(const float* __restrict__ base, int n, int pos, int D) {
  return base + (size_t)(pos < n ? pos : 0) * D;
}

// this wave's 32 x 32: acc[u][v] = the 16 x 16 products of rows i_base + 16 u + .. of a with rows j_base + 16 v + .. of b
__device__ __forceinline__ void knn_gram(const float* __restrict__ a, int na, int i_base, const float* __restrict__ b, int nb,
                                         int j_base, int D, bool vec, int lane, mfma_d4 (&acc)[2][2]) {
  const int c = lane & 15;
  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    pa[u] = knn_row(a, na, i_base + u * 16 + c, D);
    pb[u] = knn_row(b, nb, j_base + u * 16 + c, D);
  }
  gram_tile_32x32(pa[0], pa[1], pb[0], pb[1], D, vec, lane >> 4, acc);
}

// |a|^2 + |b|^2 - 2 a.b clamped at 0; NaN (a non-finite row) stays NaN
__device__ __forceinline__ double knn_dist2(double na, double nb, double dot) {
  const double d = (na + nb) - 2.0 * dot;
  return d < 0.0 ? 0.0 : d;
}

// ---- selection --------------------------------------------------------------------------------------------------------
// l ascending; keeps the KL smallest values seen.  NaN never enters (v < x is false), +inf is the empty slot.
template <int KL>
__device__ __forceinline__ void knn_insert(double (&l)[KL], double v) {
  if (v < l[KL - 1]) {
#pragma unroll
    for (int t = 0; t < KL; ++t) {
      const double lo = v < l[t] ? v : l[t], hi = v < l[t] ? l[t] : v;
      l[t] = lo, v = hi;
    }
  }
}

// grid (row blocks, chunks)
template <int KL>
__global__ __launch_bounds__(256) void knn_radii_kernel(const float* __restrict__ x, int n, int D, int k,
                                                        const double* __restrict__ norm, int T, int chunk_tiles, int n_chunks,
                                                        int vec, double* __restrict__ part) {
  __shared__ double tile[KNN_TILE * KNN_LDS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int ti = blockIdx.x, chunk = blockIdx.y;
  const int t0 = chunk * chunk_tiles, t1 = t0 + chunk_tiles < T ? t0 + chunk_tiles : T;
  const int li_base = (wave >> 1) * 32, lj_base = (wave & 1) * 32;
  const int i_base = ti * KNN_TILE + li_base;
  double na[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i_base + u * 16 + g + 4 * q;          // row (lane >> 4) + 4 q of the accumulator
      na[u][q] = i < n ? norm[i] : 0.0;
    }
  const int srow = tid >> 2, sp = tid & 3;
  double list[KL];
#pragma unroll
  for (int t = 0; t < KL; ++t) list[t] = (double)INFINITY;

  for (int tj = t0; tj < t1; ++tj) {
    const int j_base = tj * KNN_TILE + lj_base;
    mfma_d4 acc[2][2];
    knn_gram(x, n, i_base, x, n, j_base, D, vec != 0, lane, acc);
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int j = j_base + v * 16 + c;
      const double nb = j < n ? norm[j] : 0.0;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i_base + u * 16 + g + 4 * q;
          double d = knn_dist2(na[u][q], nb, acc[u][v][q]);
          if (i >= n || j >= n || i == j) d = (double)INFINITY;       // the ragged edge; self by position
          tile[(li_base + u * 16 + g + 4 * q) * KNN_LDS_STRIDE + lj_base + v * 16 + c] = d;
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KNN_TILE / 4; ++s) knn_insert<KL>(list, tile[srow * KNN_LDS_STRIDE + 4 * s + sp]);
    __syncthreads();
  }

  // the four lists of a row -> one (the tile is free: the loop ends on a barrier)
#pragma unroll
  for (int t = 0; t < KL; ++t) tile[(srow * 4 + sp) * KL + t] = list[t];
  __syncthreads();
  if (sp != 0) return;
  for (int p = 1; p < 4; ++p)
#pragma unroll
    for (int t = 0; t < KL; ++t) knn_insert<KL>(list, tile[(srow * 4 + p) * KL + t]);
  const int i = ti * KNN_TILE + srow;
  if (i >= n) return;
  double* out = part + ((size_t)i * n_chunks + chunk) * k;
#pragma unroll
  for (int t = 0; t < KL; ++t)
    if (t < k) out[t] = list[t];
}

// a thread per row: the partial lists in chunk order, then the k-th value
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ part, const double* __restrict__ norm, int n,
                                                        int k, int n_chunks, double* __restrict__ radii2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double list[HIM_KNN_MAX_K];
#pragma unroll
  for (int t = 0; t < HIM_KNN_MAX_K; ++t) list[t] = (double)INFINITY;
  const double* p = part + (size_t)i * n_chunks * k;
  for (int e = 0; e < n_chunks * k; ++e) knn_insert<HIM_KNN_MAX_K>(list, p[e]);
  double r = (double)INFINITY;
#pragma unroll
  for (int t = 0; t < HIM_KNN_MAX_K; ++t)
    if (t == k - 1) r = list[t];
  const double own = norm[i];
  radii2[i] = own != own ? (double)NAN : r;
}

// ---- membership -------------------------------------------------------------------------------------------------------
// grid (query blocks, split); workgroup (bi, s) takes the reference tiles s, s + split, ...
__global__ __launch_bounds__(256) void knn_member_kernel(const float* __restrict__ qm, int nq, const float* __restrict__ rm, int nr,
                                                         int D, const double* __restrict__ qnorm,
                                                         const double* __restrict__ rnorm, const double* __restrict__ radii2,
                                                         int Tr, int vec, int* __restrict__ row_count,
                                                         int* __restrict__ col_count) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int i_base = blockIdx.x * KNN_TILE + (wave >> 1) * 32;
  double na[2][4];
  int rows[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i_base + u * 16 + g + 4 * q;
      na[u][q] = i < nq ? qnorm[i] : 0.0;
      rows[u][q] = 0;
    }
  for (int tj = blockIdx.y; tj < Tr; tj += gridDim.y) {
    const int j_base = tj * KNN_TILE + (wave & 1) * 32;
    mfma_d4 acc[2][2];
    knn_gram(qm, nq, i_base, rm, nr, j_base, D, vec != 0, lane, acc);
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int j = j_base + v * 16 + c;
      const bool jin = j < nr;
      const double nb = jin ? rnorm[j] : 0.0, rad = jin ? radii2[j] : 0.0;
      int cols = 0;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i_base + u * 16 + g + 4 * q;
          const int in = (jin && i < nq && knn_dist2(na[u][q], nb, acc[u][v][q]) <= rad) ? 1 : 0;
          rows[u][q] += in, cols += in;
        }
      cols += __shfl_xor(cols, 16, 64);                   // the four row groups of a column
      cols += __shfl_xor(cols, 32, 64);
      if (col_count && g == 0 && jin && cols) atomicAdd(col_count + j, cols);
    }
  }
  if (!row_count) return;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int s = rows[u][q];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);     // the sixteen columns of a row
      const int i = i_base + u * 16 + g + 4 * q;
      if (c == 0 && i < nq && s) atomicAdd(row_count + i, s);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static inline bool knn_radii_shape_ok(long long n, int D, int k) {
  return k >= 1 && k <= HIM_KNN_MAX_K && n > k && n <= 0x7FFFFFFFLL && D >= 1 && D <= HIM_FEAT_MAX_DIM;
}
static inline bool knn_member_shape_ok(long long nq, long long nr, int D) {
  return nq >= 1 && nq <= 0x7FFFFFFFLL && nr >= 1 && nr <= 0x7FFFFFFFLL && D >= 1 && D <= HIM_FEAT_MAX_DIM;
}
// tiles per chunk and the number of chunks of n columns
static inline int knn_chunks(long long n, int* chunk_tiles) {
  const int T = cdiv(n, KNN_TILE);
  const int by_cap = cdiv(T, KNN_MAX_CHUNKS);
  *chunk_tiles = by_cap > KNN_CHUNK_TILES ? by_cap : KNN_CHUNK_TILES;
  return cdiv(T, *chunk_tiles);
}
static inline size_t knn_radii_ws_bytes(long long n, int k) {
  int ct;
  const size_t chunks = (size_t)knn_chunks(n, &ct);
  return ((size_t)n + (size_t)n * chunks * (size_t)k) * sizeof(double);
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_knn_radii_ws(long long n, int D, int k) { return knn_radii_shape_ok(n, D, k) ? knn_radii_ws_bytes(n, k) : 0; }

int him_knn_radii(const float* x, long long n, int D, int k, double* radii2, int* status, void* ws, size_t ws_bytes,
                  void* stream) {
  if (k < 1 || k > HIM_KNN_MAX_K) return fail(HIM_E_INVALID, "knn_radii: k %d outside 1..%d", k, HIM_KNN_MAX_K);
  if (D < 1 || D > HIM_FEAT_MAX_DIM) return fail(HIM_E_INVALID, "knn_radii: D %d outside 1..%d", D, HIM_FEAT_MAX_DIM);
  if (n <= k || n > 0x7FFFFFFFLL) return fail(HIM_E_INVALID, "knn_radii: n %lld (k %d < n <= 2^31 - 1)", n, k);
  if (!x || !radii2 || !status || !ws) return fail(HIM_E_INVALID, "knn_radii: null pointer (x, radii2, status or ws)");
  if ((uintptr_t)x % 4 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)radii2 % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID, "knn_radii: a pointer (x, radii2, status, ws) is not aligned to its element size");
  const size_t need = knn_radii_ws_bytes(n, k);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "knn_radii: workspace ws_bytes %zu < %zu bytes", ws_bytes, need);
  int chunk_tiles;
  const int n_chunks = knn_chunks(n, &chunk_tiles);
  const int T = cdiv(n, KNN_TILE), ni = (int)n;
  const int vec = gram_vec_ok(D, x, x);
  double* norm = (double*)ws;
  double* part = norm + n;
  hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, ST, x, ni, D, norm, (int*)nullptr, status);
  const dim3 grid((unsigned)T, (unsigned)n_chunks);
  if (k <= 4)
    hipLaunchKernelGGL(knn_radii_kernel<4>, grid, dim3(256), 0, ST, x, ni, D, k, norm, T, chunk_tiles, n_chunks, vec, part);
  else if (k <= 8)
    hipLaunchKernelGGL(knn_radii_kernel<8>, grid, dim3(256), 0, ST, x, ni, D, k, norm, T, chunk_tiles, n_chunks, vec, part);
  else
    hipLaunchKernelGGL(knn_radii_kernel<16>, grid, dim3(256), 0, ST, x, ni, D, k, norm, T, chunk_tiles, n_chunks, vec, part);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, ST, part, norm, ni, k, n_chunks, radii2);
  return check_launch("knn_radii");
}

size_t him_knn_membership_ws(long long nq, long long nr, int D) {
  return knn_member_shape_ok(nq, nr, D) ? (size_t)(nq + nr) * sizeof(double) : 0;
}

int him_knn_membership(const float* q, long long nq, const float* r, long long nr, int D, const double* radii2, int* row_count,
                       int* col_count, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (D < 1 || D > HIM_FEAT_MAX_DIM) return fail(HIM_E_INVALID, "knn_membership: D %d outside 1..%d", D, HIM_FEAT_MAX_DIM);
  if (nq < 1 || nq > 0x7FFFFFFFLL || nr < 1 || nr > 0x7FFFFFFFLL)
    return fail(HIM_E_INVALID, "knn_membership: nq %lld, nr %lld (each 1..2^31 - 1)", nq, nr);
  if (!q || !r || !radii2 || !status || !ws)
    return fail(HIM_E_INVALID, "knn_membership: null pointer (q, r, radii2, status or ws)");
  if (!row_count && !col_count) return fail(HIM_E_INVALID, "knn_membership: row_count and col_count are both null");
  if ((uintptr_t)q % 4 != 0 || (uintptr_t)r % 4 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)row_count % 4 != 0 ||
      (uintptr_t)col_count % 4 != 0 || (uintptr_t)radii2 % 8 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(HIM_E_INVALID,
                "knn_membership: a pointer (q, r, radii2, row_count, col_count, status, ws) is not aligned to its element size");
  const size_t need = (size_t)(nq + nr) * sizeof(double);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "knn_membership: workspace ws_bytes %zu < %zu bytes", ws_bytes, need);
  const int Tq = cdiv(nq, KNN_TILE), Tr = cdiv(nr, KNN_TILE);
  const int vec = gram_vec_ok(D, q, r);
  double* qnorm = (double*)ws;
  double* rnorm = qnorm + nq;
  hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, ST, q, (int)nq, D, qnorm, row_count, status);
  hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)cdiv(nr, 4)), dim3(256), 0, ST, r, (int)nr, D, rnorm, col_count, status);
  hipLaunchKernelGGL(knn_member_kernel, dim3((unsigned)Tq, (unsigned)(Tr < KNN_MEMBER_SPLIT ? Tr : KNN_MEMBER_SPLIT)), dim3(256), 0,
                     ST, q, (int)nq, r, (int)nr, D, qnorm, rnorm, radii2, Tr, vec, row_count, col_count);
  return check_launch("knn_membership");
}

}  // extern "C"
