// Region Poisson clone (include/him.h "Region Poisson clone"): Poisson image editing of a patch P into the photograph O
// on an ARBITRARY pixel set of a paste window, the photograph being Dirichlet data all around the set.  The membrane of
// csrc/him_membrane.hip is a direct solve and needs a rectangle; an object's outline needs an iterative one: conjugate
// gradients on the correction u = f - P, which is 0 outside the unknown set Omega.  All vectors and scalars are fp64; the
// three channels share the matrix and run in lockstep, each with its own scalars; a channel that has reached rtol is
// frozen: nothing of it is read or written again.
//
// Launches of him_region_poisson_solve, all on the caller's stream, no host read in between:
//   init    dg (uint8: deg(p) on Omega, 0 elsewhere), r := b, u := 0, the direction buffer the first step reads := 0;
//           per workgroup the partial b.b of each channel and the counts |Omega| / region pixels on the ring / non-finite
//           values read; workgroup 0 resets the record of scalars.
//   dir(k)  iteration k, first half.  Every workgroup adds the partials of r.r (written by upd(k-1), or by init) in one
//           fixed order, so all of them hold the same r.r, take the same stop decision and the same
//           beta = r.r / (r.r of the step before); workgroup 0 records r.r and the stop.  Then, fused: the new direction
//           p = r + beta p_old at the pixel AND at its four neighbours (p_old is the other of two direction buffers, so no
//           workgroup reads what another one writes in this launch), the stencil A p = deg p - sum of the neighbours' p,
//           and the partials of p.Ap.  p and r are planes that are 0 outside Omega: the stencil tests no membership.
//   upd(k)  iteration k, second half.  Every workgroup adds the partials of p.Ap, alpha = r.r / p.Ap; fused:
//           u += alpha p, r -= alpha A p and the partials of the new r.r (into the other of two partial arrays).
//   finish  one workgroup: the stop test once more after the last step, then status and resid.
// Two launches per iteration.  An iteration boundary is a kernel boundary: no workgroup waits for another one inside a
// launch.  The stop state is one int per channel, done_at, written once (by workgroup 0 of dir(k), value k) and compared
// so that a reader of the same launch sees the same truth before and after the write (done_at < k).  Once done_at < k for
// all three channels a launch returns after loading those three ints.
//
// Sums: a thread adds its pixels in tile order, block_sum_f64 adds the workgroup, and every reader adds the workgroups'
// partials as thread t: t, t + 256, ... then block_sum_f64.  No floating-point atomics, no integer atomics either:
// results are bit-identical from run to run.  p = fma(beta, p_old, r) is written as fma wherever it is evaluated, so the
// owner of a pixel and its neighbours hold the same bits.
//
// Tile: a 256-thread workgroup owns 64 columns x 4 rows, lane = column, a wave per row, the three channels in one
// thread; at most RP_MAX_BLOCKS workgroups, which take the tiles in strides, so the partial arrays have a fixed size.
// All stores are plain vector stores.  The working set of a joint-edit window (256 x 256: 1.5 MB per fp64 vector, five
// of them) lives in L2; the cost of a solve is its launches.
#include "him_common.h"

namespace him {

#define RP_TW 64
#define RP_TH 4
#define RP_MAX_N HIM_REGION_POISSON_MAX_N
#define RP_MAX_ITER HIM_REGION_POISSON_MAX_ITER
#define RP_MAX_BLOCKS 1024
#define RP_LIVE 0x7fffffff
#define RP_SPECIAL (HIM_REGION_POISSON_EMPTY | HIM_REGION_POISSON_SINGULAR | HIM_REGION_POISSON_NONFINITE)

struct RpGeom {
  int Hc, Wc, x0, y0, H, W;
  int l, r, t, b;  // the counted sides
  int tiles_x, tiles, nblk;
};

// the record of scalars at the head of the workspace
struct RpState {
  double bb[3];     // b.b
  double rr[2][3];  // r.r at the start of iteration k in slot k & 1; of a stopped channel: its last one, slot done_at & 1
  int done_at[3];   // the iteration at whose start the channel stopped = the iterations it ran; RP_LIVE until then
  int brk[3];       // p.Ap was not positive: the channel stops at the next dir
  int n_omega, n_ring, n_bad, flags;
  int pad[4];
};
static_assert(sizeof(RpState) == 128, "RpState");

struct RpHead {
  double rr[3], bb[3];
  int was[3], stop[3];
  int n_omega, n_ring, n_bad, flags;
};

// bytes: record | partials of r.r (2 x 3 x RP_MAX_BLOCKS) | of p.Ap (3 x) | int partials (3 x, as 4 bytes) | r, p0, p1, Ap
// (3 H W doubles each) | dg (H W bytes)
__host__ __device__ inline long long rp_off_part_rr() { return (long long)sizeof(RpState); }
__host__ __device__ inline long long rp_off_part_pap() { return rp_off_part_rr() + 2LL * 3 * RP_MAX_BLOCKS * 8; }
__host__ __device__ inline long long rp_off_ipart() { return rp_off_part_pap() + 3LL * RP_MAX_BLOCKS * 8; }
__host__ __device__ inline long long rp_off_planes() { return rp_off_ipart() + 3LL * RP_MAX_BLOCKS * 4; }
__host__ __device__ inline long long rp_ws_bytes(int H, int W) {
  const long long n = (long long)H * W;
  return rp_off_planes() + 4LL * 3 * n * 8 + (n + 7) / 8 * 8;
}

__device__ __forceinline__ int rp_load_done(const RpState* st, int c) {
  return __hip_atomic_load(&st->done_at[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool rp_on_ring(const RpGeom& g, int x, int y) {
  return (g.l && x == 0) || (g.r && x == g.W - 1) || (g.t && y == 0) || (g.b && y == g.H - 1);
}

// pixel of tile `tile` owned by this thread; false when it lies outside the window
__device__ __forceinline__ bool rp_pixel(const RpGeom& g, int tile, int* x, int* y) {
  *x = (tile % g.tiles_x) * RP_TW + (int)(threadIdx.x & 63);
  *y = (tile / g.tiles_x) * RP_TH + (int)(threadIdx.x >> 6);
  return *x < g.W && *y < g.H;
}

// ---- init -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    rp_init_kernel(RpGeom g, int mixed, const float* __restrict__ canvas, const float* __restrict__ P,
                   const unsigned char* __restrict__ region, double* __restrict__ u, RpState* __restrict__ st,
                   double* __restrict__ part_rr, int* __restrict__ ipart, double* __restrict__ r, double* __restrict__ p1,
                   unsigned char* __restrict__ dg) {
  __shared__ double sh[4];
  __shared__ int shi[4];
  const int n = g.H * g.W;
  double acc[3] = {0.0, 0.0, 0.0};
  int n_omega = 0, n_ring = 0, n_bad = 0;
  for (int tile = blockIdx.x; tile < g.tiles; tile += g.nblk) {
    int x, y;
    if (!rp_pixel(g, tile, &x, &y)) continue;
    const int idx = y * g.W + x;
    const bool reg = region[idx] != 0, ring = rp_on_ring(g, x, y), om = reg && !ring;
    n_ring += reg && ring;
    n_omega += om;
    // the neighbours inside the window, in the order up, down, left, right
    const int qx[4] = {x, x, x - 1, x + 1}, qy[4] = {y - 1, y + 1, y, y};
    bool qin[4], qom[4];
    int deg = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qin[j] = qx[j] >= 0 && qx[j] < g.W && qy[j] >= 0 && qy[j] < g.H;
      qom[j] = false;
      if (om && qin[j]) {
        ++deg;
        qom[j] = region[qy[j] * g.W + qx[j]] != 0 && !rp_on_ring(g, qx[j], qy[j]);
      }
    }
    dg[idx] = om ? (unsigned char)deg : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double b = 0.0;
      if (om) {
        const float* Pc = P + (long long)c * n;
        const float* Oc = canvas + ((long long)c * g.Hc + g.y0) * g.Wc + g.x0;
        const float Pp = Pc[idx];
        bool bad = !isfinite(Pp);
        double Op = 0.0;
        if (mixed) {
          const float o = Oc[(long long)y * g.Wc + x];
          bad |= !isfinite(o);
          Op = (double)o;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!qin[j]) continue;
          const float Pq = Pc[qy[j] * g.W + qx[j]];
          bad |= !isfinite(Pq);
          if (!qom[j] || mixed) {
            const float Oq = Oc[(long long)qy[j] * g.Wc + qx[j]];
            bad |= !isfinite(Oq);
            if (!qom[j]) b += (double)Oq - (double)Pq;  // Dirichlet data of the correction
            if (mixed) {
              const double dO = Op - (double)Oq, dP = (double)Pp - (double)Pq;
              if (fabs(dO) > fabs(dP)) b += dO - dP;  // ties keep the patch's gradient
            }
          }
        }
        n_bad += bad;
      }
      const int i = c * n + idx;
      r[i] = b, u[i] = 0.0, p1[i] = 0.0;
      acc[c] += b * b;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = block_sum_f64(acc[c], sh);
    if (threadIdx.x == 0) part_rr[c * RP_MAX_BLOCKS + blockIdx.x] = s;
  }
  const int counts[3] = {n_omega, n_ring, n_bad};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int s = block_sum_i32(counts[c], shi);
    if (threadIdx.x == 0) ipart[c * RP_MAX_BLOCKS + blockIdx.x] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      st->bb[c] = 0.0, st->rr[0][c] = 0.0, st->rr[1][c] = 0.0;
      st->done_at[c] = RP_LIVE, st->brk[c] = 0;
    }
    st->n_omega = st->n_ring = st->n_bad = st->flags = 0;
  }
}

// ---- the head of dir(k) and of finish: r.r, b.b and the stop decision of every channel, the same in every workgroup ----
__device__ __forceinline__ void rp_head(const RpGeom& g, int k, double rtol2, const RpState* st, const double* part_rr,
                                        const int* ipart, double* sh, int* shi, RpHead* h) {
  const double* pr = part_rr + (long long)(k & 1) * 3 * RP_MAX_BLOCKS;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = 0.0;
    for (int i = threadIdx.x; i < g.nblk; i += 256) s += pr[c * RP_MAX_BLOCKS + i];
    h->rr[c] = block_sum_f64(s, sh);
  }
  if (k == 0) {
    int cnt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int s = 0;
      for (int i = threadIdx.x; i < g.nblk; i += 256) s += ipart[c * RP_MAX_BLOCKS + i];
      cnt[c] = block_sum_i32(s, shi);
    }
    h->n_omega = cnt[0], h->n_ring = cnt[1], h->n_bad = cnt[2];
    h->flags = 0;
    if (cnt[0] == 0) h->flags |= HIM_REGION_POISSON_EMPTY;
    if (cnt[0] == g.H * g.W && !(g.l | g.r | g.t | g.b)) h->flags |= HIM_REGION_POISSON_SINGULAR;
    if (cnt[2] > 0) h->flags |= HIM_REGION_POISSON_NONFINITE;
  } else {
    h->n_omega = st->n_omega, h->n_ring = st->n_ring, h->n_bad = st->n_bad, h->flags = st->flags;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int da = rp_load_done(st, c);
    h->was[c] = da < k;
    h->bb[c] = k == 0 ? h->rr[c] : st->bb[c];
    if (h->was[c]) h->rr[c] = st->rr[da & 1][c];
    // b.b == 0 gives r.r == 0 <= 0: the channel stops before any division
    h->stop[c] = h->was[c] || (h->flags & RP_SPECIAL) != 0 || st->brk[c] != 0 || h->rr[c] <= rtol2 * h->bb[c];
  }
}

// ---- dir(k): stop decision, beta, p = r + beta p_old, A p, partials of p.Ap -------------------------------------------
__global__ void __launch_bounds__(256)
    rp_dir_kernel(RpGeom g, int k, double rtol2, RpState* __restrict__ st, const double* __restrict__ part_rr,
                  const int* __restrict__ ipart, double* __restrict__ part_pap, const double* __restrict__ r,
                  const double* __restrict__ pold, double* __restrict__ pnew, double* __restrict__ Ap,
                  const unsigned char* __restrict__ dg) {
  if (rp_load_done(st, 0) < k && rp_load_done(st, 1) < k && rp_load_done(st, 2) < k) return;
  __shared__ double sh[4];
  __shared__ int shi[4];
  RpHead h;
  rp_head(g, k, rtol2, st, part_rr, ipart, sh, shi, &h);
  double beta[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) beta[c] = (k == 0 || h.stop[c]) ? 0.0 : h.rr[c] / st->rr[(k - 1) & 1][c];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (h.was[c]) continue;
      st->rr[k & 1][c] = h.rr[c];
      if (h.stop[c]) __hip_atomic_store(&st->done_at[c], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (k == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) st->bb[c] = h.bb[c];
      st->n_omega = h.n_omega, st->n_ring = h.n_ring, st->n_bad = h.n_bad, st->flags = h.flags;
    }
  }
  if (h.stop[0] && h.stop[1] && h.stop[2]) return;
  const int n = g.H * g.W;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int tile = blockIdx.x; tile < g.tiles; tile += g.nblk) {
    int x, y;
    if (!rp_pixel(g, tile, &x, &y)) continue;
    const int idx = y * g.W + x;
    const int d = dg[idx];
    const bool up = y > 0, dn = y < g.H - 1, lf = x > 0, rt = x < g.W - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (h.stop[c]) continue;
      const int i = c * n + idx;
      if (!d) {
        pnew[i] = 0.0, Ap[i] = 0.0;
        continue;
      }
      const double bt = beta[c];
      const double pc = fma(bt, pold[i], r[i]);
      double s = 0.0;
      if (up) s += fma(bt, pold[i - g.W], r[i - g.W]);
      if (dn) s += fma(bt, pold[i + g.W], r[i + g.W]);
      if (lf) s += fma(bt, pold[i - 1], r[i - 1]);
      if (rt) s += fma(bt, pold[i + 1], r[i + 1]);
      const double ap = (double)d * pc - s;
      pnew[i] = pc, Ap[i] = ap;
      acc[c] += pc * ap;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = block_sum_f64(acc[c], sh);
    if (threadIdx.x == 0 && !h.stop[c]) part_pap[c * RP_MAX_BLOCKS + blockIdx.x] = s;
  }
}

// ---- upd(k): alpha, u += alpha p, r -= alpha A p, partials of the new r.r -----------------------------------------------
__global__ void __launch_bounds__(256)
    rp_upd_kernel(RpGeom g, int k, RpState* __restrict__ st, const double* __restrict__ part_pap,
                  double* __restrict__ part_rr, double* __restrict__ u, double* __restrict__ r,
                  const double* __restrict__ p, const double* __restrict__ Ap, const unsigned char* __restrict__ dg) {
  int done[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) done[c] = st->done_at[c] <= k;  // nobody writes done_at during an upd
  if (done[0] && done[1] && done[2]) return;
  __shared__ double sh[4];
  double alpha[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = 0.0;
    for (int i = threadIdx.x; i < g.nblk; i += 256) s += part_pap[c * RP_MAX_BLOCKS + i];
    const double pap = block_sum_f64(s, sh);
    const bool ok = !done[c] && pap > 0.0;
    alpha[c] = ok ? st->rr[k & 1][c] / pap : 0.0;
    if (!done[c] && !ok && blockIdx.x == 0 && threadIdx.x == 0) st->brk[c] = 1;
  }
  double* out = part_rr + (long long)((k + 1) & 1) * 3 * RP_MAX_BLOCKS;
  const int n = g.H * g.W;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int tile = blockIdx.x; tile < g.tiles; tile += g.nblk) {
    int x, y;
    if (!rp_pixel(g, tile, &x, &y)) continue;
    const int idx = y * g.W + x;
    if (!dg[idx]) continue;  // u, r and p are 0 there and stay so
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (done[c]) continue;
      const int i = c * n + idx;
      u[i] = fma(alpha[c], p[i], u[i]);
      const double rn = fma(-alpha[c], Ap[i], r[i]);
      r[i] = rn;
      acc[c] += rn * rn;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = block_sum_f64(acc[c], sh);
    if (threadIdx.x == 0 && !done[c]) out[c * RP_MAX_BLOCKS + blockIdx.x] = s;
  }
}

// ---- finish: one workgroup ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    rp_finish_kernel(RpGeom g, int max_iter, double rtol2, const RpState* __restrict__ st,
                     const double* __restrict__ part_rr, const int* __restrict__ ipart, int* __restrict__ status,
                     double* __restrict__ resid) {
  __shared__ double sh[4];
  __shared__ int shi[4];
  RpHead h;
  rp_head(g, max_iter, rtol2, st, part_rr, ipart, sh, shi, &h);
  if (threadIdx.x != 0) return;
  const bool special = (h.flags & RP_SPECIAL) != 0;
  int iters = 0, flags = h.flags;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int it = h.was[c] ? st->done_at[c] : max_iter;
    iters = it > iters ? it : iters;
    const bool reached = h.rr[c] <= rtol2 * h.bb[c];
    if (!special && !reached) flags |= HIM_REGION_POISSON_MAX_ITER_HIT;
    resid[c] = (special || !(h.bb[c] > 0.0)) ? 0.0 : sqrt(h.rr[c] / h.bb[c]);
  }
  status[0] = g.l | (g.r << 1) | (g.t << 2) | (g.b << 3);
  status[1] = h.n_omega, status[2] = h.n_ring, status[3] = iters, status[4] = flags;
  status[5] = status[6] = status[7] = 0;
}

// ---- apply ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    rp_apply_kernel(RpGeom g, const float* __restrict__ P, const double* __restrict__ u,
                    const unsigned char* __restrict__ region, float* __restrict__ canvas) {
  const int n = g.H * g.W;
  for (int tile = blockIdx.x; tile < g.tiles; tile += g.nblk) {
    int x, y;
    if (!rp_pixel(g, tile, &x, &y)) continue;
    const int idx = y * g.W + x;
    if (region[idx] == 0 || rp_on_ring(g, x, y)) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = (float)((double)P[c * n + idx] + u[c * n + idx]);  // the only fp32 rounding of the sum
      canvas[((long long)c * g.Hc + g.y0 + y) * g.Wc + g.x0 + x] = fminf(fmaxf(v, 0.f), 1.f);
    }
  }
}

static inline bool rp_geometry(int Hc, int Wc, int x0, int y0, int H, int W, RpGeom* g) {
  if (H < 1 || W < 1 || H > RP_MAX_N || W > RP_MAX_N) return false;
  if (x0 < 0 || y0 < 0 || (long long)x0 + W > Wc || (long long)y0 + H > Hc) return false;
  g->Hc = Hc, g->Wc = Wc, g->x0 = x0, g->y0 = y0, g->H = H, g->W = W;
  g->l = x0 > 0, g->r = x0 + W < Wc, g->t = y0 > 0, g->b = y0 + H < Hc;
  g->tiles_x = cdiv(W, RP_TW);
  g->tiles = g->tiles_x * cdiv(H, RP_TH);
  g->nblk = g->tiles < RP_MAX_BLOCKS ? g->tiles : RP_MAX_BLOCKS;
  return true;
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_region_poisson_ws(int H, int W) {
  if (H < 1 || W < 1 || H > RP_MAX_N || W > RP_MAX_N) return 0;
  return (size_t)rp_ws_bytes(H, W);
}

int him_region_poisson_solve(const float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const float* P,
                             const unsigned char* region, int mixed, double rtol, int max_iter, double* u, int* status,
                             double* resid, void* ws, size_t ws_bytes, void* stream) {
  if (!canvas || !P || !region || !u || !status || !resid) return fail(HIM_E_INVALID, "region_poisson_solve: null pointer");
  if (H < 1 || W < 1 || H > RP_MAX_N || W > RP_MAX_N)
    return fail(HIM_E_INVALID, "region_poisson_solve: window %dx%d outside 1..%d per axis", W, H, RP_MAX_N);
  RpGeom g;
  if (!rp_geometry(Hc, Wc, x0, y0, H, W, &g))
    return fail(HIM_E_INVALID, "region_poisson_solve: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc, Hc);
  if (mixed != 0 && mixed != 1) return fail(HIM_E_INVALID, "region_poisson_solve: mixed %d", mixed);
  if (!(rtol > 0.0 && rtol < 1.0)) return fail(HIM_E_INVALID, "region_poisson_solve: rtol %g outside (0, 1)", rtol);
  if (max_iter < 1 || max_iter > RP_MAX_ITER)
    return fail(HIM_E_INVALID, "region_poisson_solve: max_iter %d outside 1..%d", max_iter, RP_MAX_ITER);
  if ((uintptr_t)u % 8 || (uintptr_t)resid % 8) return fail(HIM_E_INVALID, "region_poisson_solve: u and resid are fp64 arrays");
  if (!ws) return fail(HIM_E_WORKSPACE, "region_poisson_solve: null workspace");
  if ((uintptr_t)ws % 8) return fail(HIM_E_INVALID, "region_poisson_solve: workspace not aligned to 8 bytes");
  if (ws_bytes < (size_t)rp_ws_bytes(H, W))
    return fail(HIM_E_WORKSPACE, "region_poisson_solve: workspace of %zu bytes, %lld needed", ws_bytes, rp_ws_bytes(H, W));
  char* w = (char*)ws;
  RpState* st = (RpState*)w;
  double* part_rr = (double*)(w + rp_off_part_rr());
  double* part_pap = (double*)(w + rp_off_part_pap());
  int* ipart = (int*)(w + rp_off_ipart());
  const long long n3 = 3LL * H * W;
  double* r = (double*)(w + rp_off_planes());
  double* pb[2] = {r + n3, r + 2 * n3};
  double* Ap = r + 3 * n3;
  unsigned char* dg = (unsigned char*)(Ap + n3);
  const double rtol2 = rtol * rtol;
  const dim3 grid(g.nblk), block(256);
  hipLaunchKernelGGL(rp_init_kernel, grid, block, 0, ST, g, mixed, canvas, P, region, u, st, part_rr, ipart, r, pb[1], dg);
  for (int k = 0; k < max_iter; ++k) {
    hipLaunchKernelGGL(rp_dir_kernel, grid, block, 0, ST, g, k, rtol2, st, (const double*)part_rr, (const int*)ipart,
                       part_pap, (const double*)r, (const double*)pb[(k & 1) ^ 1], pb[k & 1], Ap, (const unsigned char*)dg);
    hipLaunchKernelGGL(rp_upd_kernel, grid, block, 0, ST, g, k, st, (const double*)part_pap, part_rr, u, r,
                       (const double*)pb[k & 1], (const double*)Ap, (const unsigned char*)dg);
  }
  hipLaunchKernelGGL(rp_finish_kernel, dim3(1), block, 0, ST, g, max_iter, rtol2, (const RpState*)st,
                     (const double*)part_rr, (const int*)ipart, status, resid);
  return check_launch("region_poisson_solve");
}

int him_region_poisson_apply(const float* P, const double* u, const unsigned char* region, float* canvas, int Hc, int Wc,
                             int x0, int y0, int H, int W, void* stream) {
  if (!P || !u || !region || !canvas) return fail(HIM_E_INVALID, "region_poisson_apply: null pointer");
  if (H < 1 || W < 1 || H > RP_MAX_N || W > RP_MAX_N)
    return fail(HIM_E_INVALID, "region_poisson_apply: window %dx%d outside 1..%d per axis", W, H, RP_MAX_N);
  RpGeom g;
  if (!rp_geometry(Hc, Wc, x0, y0, H, W, &g))
    return fail(HIM_E_INVALID, "region_poisson_apply: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H, Wc, Hc);
  if ((uintptr_t)u % 8) return fail(HIM_E_INVALID, "region_poisson_apply: u is an fp64 array");
  hipLaunchKernelGGL(rp_apply_kernel, dim3(g.nblk), dim3(256), 0, ST, g, P, u, region, canvas);
  return check_launch("region_poisson_apply");
}

}  // extern "C"
