// The membrane of seamless (gradient-domain) compositing (include/him.h "Seamless canvas composite"): the discrete
// harmonic function m on a rectangular paste window whose boundary values are O - P on the window's ring, so that P + m
// is the Poisson clone of the patch P into the photograph O.  On a rectangle the 5-point Laplacian with Dirichlet
// (counted side) / Neumann (uncounted side) ends is diagonalised by closed-form sine / cosine bases, so the solve is
// direct:  m = Vy (Bh / (lamy_i + lamx_j)) Vx^T,  Bh = Vy^T B Vx.  B is nonzero only on the interior's outer rows and
// columns, so Bh is four matrix-vector products and a rank-4 update; only the inverse transform is two full GEMMs, and
// those run on v_mfma_f64_16x16x4_f64 (fragment layout: csrc/him_mfma_f64.h).  Everything is fp64 up to the final
// narrowing store; no atomics; every sum has one fixed order, so results are bit-identical from run to run.
//
// Launches of him_membrane_solve, all on the caller's stream:
//   ring    one thread per ring pixel and channel: g = (double)O - (double)P, m := (float)g on the ring, and the four
//           boundary vectors gT / gB (nx) and gL / gR (ny) into the workspace; thread 0 writes the status.
//   matvec  one wave per output: hT[j] = Vxt[j,:] . gT, hB likewise, hL[i] = Vyt[i,:] . gL, hR likewise.  Lane l adds
//           elements l, l + 64, ... in order, then the xor butterfly of wave_sum_f64.
//   scale   C[i,j] = (Vy[0,i] hT[j] + Vy[ny-1,i] hB[j] + hL[i] Vx[0,j] + hR[i] Vx[nx-1,j]) / (lamy[i] + lamx[j]), the
//           terms of uncounted sides dropped, added in that order.
//   gemm    T = Vy C  (ny x ny by ny x nx), then  m = T Vxt  (ny x nx by nx x nx) with the epilogue narrowing to fp32 into
//           the interior of the (3,H,W) plane; grid z = channel.
//
// GEMM tile: 256 threads own a 64 x 64 tile of the row-major product; wave w owns the 32 x 32 block (w >> 1, w & 1) as
// 2 x 2 accumulators of 16 x 16.  K advances 16 at a time through LDS: As[64][MB_LDA] (row m, k contiguous) and
// Bs[16][MB_LDB] (row k, n contiguous).  A fragment load is one ds_read_b64 per lane; its banks are (byte / 4) % 64 per
// 32-lane half, i.e. the 8-byte element index % 32 must differ over the half's 16 m (or n) x 2 k:
//   A: index m * 18 + k:  m * 18 % 32 runs over the 16 even residues, k in {g, g + 1} adds the odd ones -> conflict-free
//      (a pitch of 16 would put all 16 m on two residues: 8-way).
//   B: index k * 80 + n:  80 % 32 = 16, so the two k rows of a half take residues 0..15 and 16..31 -> conflict-free
//      (a pitch of 64 would fold both rows onto 0..15: 2-way).
// Edge tiles: loads outside the matrices are replaced by zeros, stores outside are skipped; all stores are plain vector
// stores.  The row pitches of the operands are arbitrary (ny, nx), so global loads are 8-byte loads.
#include "him_common.h"
#include "him_mfma_f64.h"

namespace him {

#define MB_MAX_N HIM_MEMBRANE_MAX_N  // largest interior side
#define MB_TM 64
#define MB_TN 64
#define MB_TK 16
#define MB_LDA 18
#define MB_LDB 80

// ---- bases ----------------------------------------------------------------------------------------------------------
// sin(pi a / p) for integers 0 <= a, p > 0: a is reduced modulo the period 2 p and folded into [0, p / 2] in integers,
// so the argument handed to sinpi is a rational in [0, 1/2] whatever the size of a.
__device__ __forceinline__ double mb_sin_ratio(long long a, long long p) {
  a %= 2 * p;
  double s = 1.0;
  if (a >= p) a -= p, s = -1.0;
  if (2 * a > p) a = p - a;
  return s * sinpi((double)a / (double)p);
}
// cos(pi a / p): period 2 p, cos(2 pi - t) = cos t, cos(pi - t) = -cos t
__device__ __forceinline__ double mb_cos_ratio(long long a, long long p) {
  a %= 2 * p;
  double s = 1.0;
  if (a > p) a = 2 * p - a;
  if (2 * a > p) a = p - a, s = -1.0;
  return s * cospi((double)a / (double)p);
}

// the unnormalised V[j][k] of the boundary pair (lo, hi) on an axis of n
__device__ __forceinline__ double mb_basis_raw(int n, int lo, int hi, int j, int k) {
  if (lo && hi) return mb_sin_ratio((long long)(k + 1) * (j + 1), n + 1);
  if (!lo && !hi) return mb_cos_ratio((long long)k * (2 * j + 1), 2LL * n);
  if (lo) return mb_sin_ratio((long long)(2 * k + 1) * (j + 1), 2LL * n + 1);
  return mb_sin_ratio((long long)(2 * k + 1) * (n - j), 2LL * n + 1);
}

// 2 - 2 cos(t) = 4 sin^2(t / 2): the same number without the cancellation at small t
__device__ __forceinline__ double mb_lambda(int n, int lo, int hi, int k) {
  double s;
  if (lo && hi) s = mb_sin_ratio(k + 1, 2LL * (n + 1));
  else if (!lo && !hi) s = mb_sin_ratio(k, 2LL * n);
  else s = mb_sin_ratio(2 * k + 1, 2LL * (2 * n + 1));
  return 4.0 * s * s;
}

// One workgroup per column k: the column's squared norm (thread t adds j = t, t + 256, ... in order, then
// block_sum_f64), then row k of Vt = the normalised column, and lam[k].
__global__ void __launch_bounds__(256) membrane_basis_kernel(int n, int lo, int hi, double* __restrict__ Vt,
                                                             double* __restrict__ lam) {
  __shared__ double sh[4];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const double v = mb_basis_raw(n, lo, hi, j, k);
    s += v * v;
  }
  const double inv = 1.0 / sqrt(block_sum_f64(s, sh));
  for (int j = threadIdx.x; j < n; j += 256) Vt[(long long)k * n + j] = mb_basis_raw(n, lo, hi, j, k) * inv;
  if (threadIdx.x == 0) lam[k] = mb_lambda(n, lo, hi, k);
}

// V = Vt^T through a 32 x 33 LDS tile: both sides move as contiguous rows
__global__ void __launch_bounds__(256) membrane_transpose_kernel(int n, const double* __restrict__ Vt,
                                                                 double* __restrict__ V) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8)
    if (r0 + r < n && c0 + tx < n) tile[r][tx] = Vt[(long long)(r0 + r) * n + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (c0 + r < n && r0 + tx < n) V[(long long)(c0 + r) * n + r0 + tx] = tile[tx][r];
}

// ---- solve ----------------------------------------------------------------------------------------------------------
struct MbGeom {
  int Hc, Wc, x0, y0, H, W;
  int t, b, l, r;  // the counted sides
  int ny, nx;
};

// per channel, in doubles: gT gB (nx each) gL gR (ny each) hT hB (nx each) hL hR (ny each) C (ny nx) T (ny nx)
__host__ __device__ inline long long mb_vec_doubles(int ny, int nx) { return 4LL * (nx + ny); }
__host__ __device__ inline long long mb_chan_doubles(int ny, int nx) { return mb_vec_doubles(ny, nx) + 2LL * ny * nx; }

// ring pixel number e of the window -> (x, y): the counted top row, the counted bottom row, then the counted left and
// right columns without the rows already listed
__device__ __forceinline__ void mb_ring_pixel(const MbGeom& g, int e, int* x, int* y) {
  if (g.t) {
    if (e < g.W) { *x = e, *y = 0; return; }
    e -= g.W;
  }
  if (g.b) {
    if (e < g.W) { *x = e, *y = g.H - 1; return; }
    e -= g.W;
  }
  if (g.l) {
    if (e < g.ny) { *x = 0, *y = g.t + e; return; }
    e -= g.ny;
  }
  *x = g.W - 1, *y = g.t + e;
}

__global__ void __launch_bounds__(256)
    membrane_ring_kernel(MbGeom g, int n_ring, const float* __restrict__ canvas, const float* __restrict__ P,
                         float* __restrict__ m, double* __restrict__ ws, int* __restrict__ status) {
  const int e = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (e == 0 && c == 0) {
    status[0] = g.l | (g.r << 1) | (g.t << 2) | (g.b << 3);
    status[1] = g.ny, status[2] = g.nx, status[3] = 0;
  }
  if (e >= n_ring) return;
  int x, y;
  mb_ring_pixel(g, e, &x, &y);
  const long long iw = ((long long)c * g.H + y) * g.W + x;
  const double d = (double)canvas[((long long)c * g.Hc + g.y0 + y) * g.Wc + g.x0 + x] - (double)P[iw];
  m[iw] = (float)d;
  double* v = ws + (long long)c * mb_chan_doubles(g.ny, g.nx);
  // a corner of the ring is nobody's neighbour: only ring pixels beside the interior enter the vectors
  const int jx = x - g.l, iy = y - g.t;
  if (g.t && y == 0 && jx >= 0 && jx < g.nx) v[jx] = d;
  if (g.b && y == g.H - 1 && jx >= 0 && jx < g.nx) v[g.nx + jx] = d;
  if (g.l && x == 0 && iy >= 0 && iy < g.ny) v[2 * g.nx + iy] = d;
  if (g.r && x == g.W - 1 && iy >= 0 && iy < g.ny) v[2 * g.nx + g.ny + iy] = d;
}

// no side counted: m := 0 over the whole window, status bit HIM_MEMBRANE_NO_SIDE
__global__ void __launch_bounds__(256)
    membrane_zero_kernel(long long n, int ny, int nx, float* __restrict__ m, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) status[0] = 0, status[1] = ny, status[2] = nx, status[3] = HIM_MEMBRANE_NO_SIDE;
  if (i < n) m[i] = 0.f;
}

// one wave per output o of channel blockIdx.y: o in [0, 2 nx): h{T,B}[j] = Vxt[j,:] . g{T,B};  o in [2 nx, 2 nx + 2 ny):
// h{L,R}[i] = Vyt[i,:] . g{L,R}.  Vectors of uncounted sides are skipped: nothing reads them.
__global__ void __launch_bounds__(256)
    membrane_matvec_kernel(MbGeom g, const double* __restrict__ Vyt, const double* __restrict__ Vxt,
                           double* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int o = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (o >= 2 * (g.nx + g.ny)) return;
  double* v = ws + (long long)blockIdx.y * mb_chan_doubles(g.ny, g.nx);
  const double *row, *vec;
  int n;
  if (o < 2 * g.nx) {
    const int side = o / g.nx, j = o % g.nx;
    if (!(side ? g.b : g.t)) return;
    n = g.nx, row = Vxt + (long long)j * g.nx, vec = v + side * g.nx;
  } else {
    const int q = o - 2 * g.nx, side = q / g.ny, i = q % g.ny;
    if (!(side ? g.r : g.l)) return;
    n = g.ny, row = Vyt + (long long)i * g.ny, vec = v + 2 * g.nx + side * g.ny;
  }
  double s = 0.0;
  for (int k = lane; k < n; k += 64) s += row[k] * vec[k];
  s = wave_sum_f64(s);
  if (lane == 0) v[2 * (g.nx + g.ny) + o] = s;
}

__global__ void __launch_bounds__(256)
    membrane_scale_kernel(MbGeom g, const double* __restrict__ Vy, const double* __restrict__ lamy,
                          const double* __restrict__ Vx, const double* __restrict__ lamx, double* __restrict__ ws) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= g.nx) return;
  double* v = ws + (long long)blockIdx.z * mb_chan_doubles(g.ny, g.nx);
  const double* h = v + 2 * (g.nx + g.ny);
  double s = 0.0;
  if (g.t) s += Vy[i] * h[j];
  if (g.b) s += Vy[(long long)(g.ny - 1) * g.ny + i] * h[g.nx + j];
  if (g.l) s += h[2 * g.nx + i] * Vx[j];
  if (g.r) s += h[2 * g.nx + g.ny + i] * Vx[(long long)(g.nx - 1) * g.nx + j];
  v[mb_vec_doubles(g.ny, g.nx) + (long long)i * g.nx + j] = s / (lamy[i] + lamx[j]);
}

// C (M x N) = A (M x K) B (K x N), row-major fp64 with pitches lda / ldb / ldc, per channel z at A + z sa, B + z sb,
// C + z sc.  OUT32: C is fp32 and the product is narrowed on the store.
template <bool OUT32>
__global__ void __launch_bounds__(256)
    membrane_gemm_kernel(int M, int N, int K, const double* __restrict__ A, int lda, long long sa,
                         const double* __restrict__ B, int ldb, long long sb, void* __restrict__ Cv, int ldc,
                         long long sc) {
  __shared__ double As[MB_TM * MB_LDA];
  __shared__ double Bs[MB_TK * MB_LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * MB_TM, n0 = blockIdx.x * MB_TN;
  A += (long long)blockIdx.z * sa;
  B += (long long)blockIdx.z * sb;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int fm = lane & 15, g = lane >> 4;
  // staging: thread -> 4 consecutive k of one A row, 4 consecutive n of one B row
  const int ar = tid >> 2, ak = (tid & 3) * 4;
  const int bk = tid >> 4, bn = (tid & 15) * 4;
  const bool a_row_ok = m0 + ar < M;
  const double* ap = A + (long long)(a_row_ok ? m0 + ar : 0) * lda;
  mfma_d4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += MB_TK) {
    double a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + ak + q;
      a[q] = (a_row_ok && k < K) ? ap[k] : 0.0;
    }
    {
      const int k = k0 + bk;
      const double* bp = B + (long long)(k < K ? k : 0) * ldb;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + bn + q;
        b[q] = (k < K && n < N) ? bp[n] : 0.0;
      }
    }
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int q = 0; q < 4; ++q) As[ar * MB_LDA + ak + q] = a[q], Bs[bk * MB_LDB + bn + q] = b[q];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * j + g;
      double fa[2], fb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) fa[u] = As[(wm + 16 * u + fm) * MB_LDA + k], fb[u] = Bs[k * MB_LDB + wn + 16 * u + fm];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[u], fb[v], acc[u][v], 0, 0, 0);
    }
  }
  // C/D register q of v_mfma_f64_16x16x4_f64: column lane & 15, row (lane >> 4) + 4 q
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + wm + 16 * u + g + 4 * q, col = n0 + wn + 16 * v + fm;
        if (row < M && col < N) {
          const long long i = (long long)blockIdx.z * sc + (long long)row * ldc + col;
          if (OUT32) ((float*)Cv)[i] = (float)acc[u][v][q];
          else ((double*)Cv)[i] = acc[u][v][q];
        }
      }
}

static inline bool mb_geometry(int Hc, int Wc, int x0, int y0, int H, int W, MbGeom* g) {
  if (H < 1 || W < 1 || x0 < 0 || y0 < 0 || (long long)x0 + W > Wc || (long long)y0 + H > Hc) return false;
  g->Hc = Hc, g->Wc = Wc, g->x0 = x0, g->y0 = y0, g->H = H, g->W = W;
  g->l = x0 > 0, g->r = x0 + W < Wc, g->t = y0 > 0, g->b = y0 + H < Hc;
  g->ny = H - g->t - g->b, g->nx = W - g->l - g->r;
  return true;
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

int him_membrane_basis(int n, int lo, int hi, double* V, double* Vt, double* lam, void* stream) {
  if (!V || !Vt || !lam) return fail(HIM_E_INVALID, "membrane_basis: null pointer");
  if (n < 1 || n > MB_MAX_N) return fail(HIM_E_INVALID, "membrane_basis: n %d outside 1..%d", n, MB_MAX_N);
  if ((lo != 0 && lo != 1) || (hi != 0 && hi != 1)) return fail(HIM_E_INVALID, "membrane_basis: flags (%d,%d)", lo, hi);
  if ((uintptr_t)V % 8 || (uintptr_t)Vt % 8 || (uintptr_t)lam % 8 || V == Vt)
    return fail(HIM_E_INVALID, "membrane_basis: V, Vt and lam are distinct fp64 arrays");
  hipLaunchKernelGGL(membrane_basis_kernel, dim3(n), dim3(256), 0, ST, n, lo, hi, Vt, lam);
  const int tiles = cdiv(n, 32);
  hipLaunchKernelGGL(membrane_transpose_kernel, dim3(tiles, tiles), dim3(256), 0, ST, n, Vt, V);
  return check_launch("membrane_basis");
}

size_t him_membrane_ws(int H, int W, int sides) {
  if (H < 1 || W < 1 || sides < 0 || sides > 15) return 0;
  const int ny = H - ((sides >> 2) & 1) - ((sides >> 3) & 1), nx = W - (sides & 1) - ((sides >> 1) & 1);
  if (ny < 1 || nx < 1 || ny > MB_MAX_N || nx > MB_MAX_N) return 0;
  return (size_t)(3 * mb_chan_doubles(ny, nx)) * sizeof(double);
}

int him_membrane_solve(const float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const float* P,
                       const double* Vy, const double* Vyt, const double* lamy, const double* Vx, const double* Vxt,
                       const double* lamx, float* m, void* ws, int* status, void* stream) {
  if (!canvas || !P || !m || !status) return fail(HIM_E_INVALID, "membrane_solve: null pointer");
  MbGeom g;
  if (!mb_geometry(Hc, Wc, x0, y0, H, W, &g))
    return fail(HIM_E_INVALID, "membrane_solve: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc, Hc);
  if (g.ny < 1 || g.nx < 1) return fail(HIM_E_INVALID, "membrane_solve: a %dx%d window has no interior (%dx%d)", W, H, g.nx, g.ny);
  if (g.ny > MB_MAX_N || g.nx > MB_MAX_N)
    return fail(HIM_E_INVALID, "membrane_solve: interior %dx%d above %d per axis", g.nx, g.ny, MB_MAX_N);
  if (!(g.t | g.b | g.l | g.r)) {
    const long long n = 3LL * H * W;
    hipLaunchKernelGGL(membrane_zero_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, ST, n, g.ny, g.nx, m, status);
    return check_launch("membrane_solve");
  }
  if (!Vy || !Vyt || !lamy || !Vx || !Vxt || !lamx) return fail(HIM_E_INVALID, "membrane_solve: null basis");
  if (!ws) return fail(HIM_E_WORKSPACE, "membrane_solve: null workspace");
  if ((uintptr_t)ws % 8) return fail(HIM_E_INVALID, "membrane_solve: workspace not aligned to 8 bytes");
  double* w = (double*)ws;
  const int ny = g.ny, nx = g.nx;
  const int n_ring = (g.t + g.b) * W + (g.l + g.r) * ny;
  const long long chan = mb_chan_doubles(ny, nx);
  hipLaunchKernelGGL(membrane_ring_kernel, dim3(cdiv(n_ring, 256), 3), dim3(256), 0, ST, g, n_ring, canvas, P, m, w, status);
  hipLaunchKernelGGL(membrane_matvec_kernel, dim3(cdiv(2 * (nx + ny), 4), 3), dim3(256), 0, ST, g, Vyt, Vxt, w);
  hipLaunchKernelGGL(membrane_scale_kernel, dim3(cdiv(nx, 256), ny, 3), dim3(256), 0, ST, g, Vy, lamy, Vx, lamx, w);
  double* C = w + mb_vec_doubles(ny, nx);
  double* T = C + (long long)ny * nx;
  const dim3 grid(cdiv(nx, MB_TN), cdiv(ny, MB_TM), 3);
  hipLaunchKernelGGL(membrane_gemm_kernel<false>, grid, dim3(256), 0, ST, ny, nx, ny, Vy, ny, 0LL, (const double*)C, nx,
                     chan, (void*)T, nx, chan);
  hipLaunchKernelGGL(membrane_gemm_kernel<true>, grid, dim3(256), 0, ST, ny, nx, nx, (const double*)T, nx, chan, Vxt, nx,
                     0LL, (void*)(m + (long long)g.t * W + g.l), W, (long long)H * W);
  return check_launch("membrane_solve");
}

}  // extern "C"
