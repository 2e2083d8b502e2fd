// Layout edits on a (label, instance) canvas pair (include/him.h "Layout edits"): take an instance out and fill the hole
// from the nearest pixel of an allowed class, and write an instance of one pair into another at another size.  Integer
// work throughout, integer atomics only (add / or / min / max commute): results are bit-identical from run to run.
//
// him_layout_erase, two launches of its own around him_edt's three:
//   init    one thread: the job row [plane 0, -, HIM_EDT_NONZERO] of the transform and a zeroed status record.
//   seeds   grid-stride, one pixel per thread and trip: region test, class lookup in the bit table; writes the uint8 seed
//           plane, the COPIES of both planes and a zeroed `changed`; counts |R| and raises the range flag, one atomic per
//           wave that has something to add.
//   him_edt over the seed plane (kind 0, one job), nearest seed wanted: the transform is him_edt.hip's, not restated here.
//   gather  grid-stride: a region pixel with a valid class and a seed reads both planes at nearest[p] and rewrites the
//           copies; counts the pixels whose class changed; one thread copies the seed count and raises the no-seed flag.
// him_layout_place, two launches: status init; a 256-thread workgroup per tile of 64 columns x 4 rows of the destination
//   box clipped to the canvas, lane = column, a pixel per thread: the source pixel through the two index tables, the
//   instance test, the protected-class lookup, three byte / word stores, and wave reductions in front of the atomics.
//
// Affine layout edits (include/him.h "Affine layout edits"): the same placement and a bicubic warp of the photograph
// through an inverse affine map in 2^-24 fixed point, six int64 coefficients in the kernel arguments.
// him_layout_place_affine: him_layout_place's two launches; the kernel computes the nearest source pixel from the map
//   where its sibling reads two tables, and hands the pixel to the same le_place_commit.
// him_canvas_warp_affine: one launch, the same 64 x 4 tiles, the three channels in one thread; sixteen clamped taps per
//   channel gathered from global memory, fp64 weights and sums, one narrowing per output, no atomics, no workspace.
#include "him_common.h"

namespace him {

#define LE_MAXDIM 16384
#define LE_MAX_CLASS 65536
#define LE_MAX_COORD (1 << 20)
#define LE_TW 64
#define LE_TH 4

__device__ __forceinline__ bool le_is(unsigned char c, int v) { return (int)c == v; }
__device__ __forceinline__ bool le_is(int c, int v) { return c == v; }
__device__ __forceinline__ bool le_is(long long c, int v) { return c == (long long)v; }
__device__ __forceinline__ bool le_is(float c, int v) { return c == (float)v; }

// the class id of a label value, -1 when it lies outside [0, n) (or is not integral)
__device__ __forceinline__ int le_class(unsigned char c, int n) { return (int)c < n ? (int)c : -1; }
__device__ __forceinline__ int le_class(int c, int n) { return (c >= 0 && c < n) ? c : -1; }
__device__ __forceinline__ int le_class(long long c, int n) { return (c >= 0 && c < (long long)n) ? (int)c : -1; }
__device__ __forceinline__ int le_class(float c, int n) {
  return (c >= 0.f && c < (float)n && c == truncf(c)) ? (int)c : -1;  // a NaN fails the first comparison
}
__device__ __forceinline__ bool le_bit(const unsigned* __restrict__ table, int c) { return (table[c >> 5] >> (c & 31)) & 1u; }

__global__ void le_erase_init_kernel(int* __restrict__ jobs, int* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    jobs[0] = 0, jobs[1] = 0, jobs[2] = HIM_EDT_NONZERO;
    status[0] = 0, status[1] = 0, status[2] = 0, status[3] = 0;
  }
}

template <typename TL, typename TI>
__global__ __launch_bounds__(256) void le_seed_kernel(const TL* __restrict__ label, const TI* __restrict__ inst,
                                                      const unsigned char* __restrict__ region, int id, long long hw,
                                                      const unsigned* __restrict__ fill, int n_class,
                                                      unsigned char* __restrict__ seeds, TL* __restrict__ label_out,
                                                      TI* __restrict__ inst_out, unsigned char* __restrict__ changed,
                                                      int* __restrict__ status) {
  int n_r = 0, n_bad = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < hw; i += (long long)gridDim.x * blockDim.x) {
    const TL l = label[i];
    const TI q = inst[i];
    const bool in_r = region ? region[i] != 0 : le_is(q, id);
    const int c = le_class(l, n_class);
    n_r += in_r ? 1 : 0;
    n_bad += c < 0 ? 1 : 0;
    seeds[i] = (!in_r && c >= 0 && le_bit(fill, c)) ? 1 : 0;
    label_out[i] = l;
    inst_out[i] = q;
    changed[i] = 0;
  }
  n_r = wave_sum_i32(n_r);
  n_bad = wave_sum_i32(n_bad);
  if ((threadIdx.x & 63) == 0) {
    if (n_r) atomicAdd(&status[0], n_r);
    if (n_bad) atomicOr(&status[3], HIM_LAYOUT_CLASS_RANGE);
  }
}

template <typename TL, typename TI>
__global__ __launch_bounds__(256) void le_gather_kernel(const TL* __restrict__ label, const TI* __restrict__ inst,
                                                        const unsigned char* __restrict__ region, int id, long long hw,
                                                        int n_class, const int* __restrict__ nearest,
                                                        const int* __restrict__ edt_status, TL* __restrict__ label_out,
                                                        TI* __restrict__ inst_out, unsigned char* __restrict__ changed,
                                                        int* __restrict__ status) {
  const int n_seed = edt_status[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[1] = n_seed;
    if (n_seed == 0) atomicOr(&status[3], HIM_LAYOUT_NO_SEED);
  }
  if (n_seed == 0) return;  // uniform: the copies stand
  int n_ch = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < hw; i += (long long)gridDim.x * blockDim.x) {
    const TL l = label[i];
    const bool in_r = region ? region[i] != 0 : le_is(inst[i], id);
    if (!in_r || le_class(l, n_class) < 0) continue;
    const int s = nearest[i];
    if (s < 0 || (long long)s >= hw) continue;  // cannot happen with a seed in the plane; never index with it
    const TL ls = label[s];
    label_out[i] = ls;
    inst_out[i] = inst[s];
    if (ls != l) changed[i] = 1, ++n_ch;
  }
  n_ch = wave_sum_i32(n_ch);
  if ((threadIdx.x & 63) == 0 && n_ch) atomicAdd(&status[2], n_ch);
}

__global__ void le_place_init_kernel(int* __restrict__ status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[0] = 0, status[1] = 0;
    status[2] = 0x7fffffff, status[3] = 0x7fffffff, status[4] = -1, status[5] = -1;
  }
}

struct LePlace {
  int Ws, id, sx0, sy0, sw, sh;       // source canvas width, instance, box origin and size
  int Wd, dx0, dy0;                   // destination canvas width, box origin (may be negative)
  int cx0, cy0, cw, chh, tiles_x;     // the clipped window and its tiling
  int cls, new_id, n_class;
};

// What both place kernels do with a destination pixel (x, y) once they know whether the resampled mask is set there
// (`hit`; false for the threads beyond the clipped window): the protected-class lookup, the three stores, the counts,
// and the wave reductions in front of the atomics.  Every thread of the wave calls it.
template <typename TL, typename TI>
__device__ __forceinline__ void le_place_commit(bool hit, int x, int y, TL* __restrict__ label_dst, TI* __restrict__ inst_dst,
                                                const unsigned* __restrict__ protect, unsigned char* __restrict__ changed,
                                                int* __restrict__ status, const LePlace& p) {
  int wrote = 0, blocked = 0, x_lo = 0x7fffffff, y_lo = 0x7fffffff, x_hi = -1, y_hi = -1;
  if (hit) {
    const size_t o = (size_t)y * p.Wd + x;
    const int c = protect ? le_class(label_dst[o], p.n_class) : -1;
    if (c >= 0 && le_bit(protect, c)) {
      blocked = 1;
    } else {
      label_dst[o] = (TL)p.cls;
      inst_dst[o] = (TI)p.new_id;
      if (changed) changed[o] = 1;
      wrote = 1, x_lo = x_hi = x, y_lo = y_hi = y;
    }
  }
  const int n_w = wave_sum_i32(wrote), n_b = wave_sum_i32(blocked);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x_lo = min(x_lo, __shfl_xor(x_lo, o, 64));
    y_lo = min(y_lo, __shfl_xor(y_lo, o, 64));
    x_hi = max(x_hi, __shfl_xor(x_hi, o, 64));
    y_hi = max(y_hi, __shfl_xor(y_hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_b) atomicAdd(&status[1], n_b);
    if (n_w) {
      atomicAdd(&status[0], n_w);
      atomicMin(&status[2], x_lo);
      atomicMin(&status[3], y_lo);
      atomicMax(&status[4], x_hi);
      atomicMax(&status[5], y_hi);
    }
  }
}

template <typename TL, typename TI>
__global__ __launch_bounds__(256) void le_place_kernel(const TI* __restrict__ inst_src, const int* __restrict__ xs,
                                                       const int* __restrict__ ys, TL* __restrict__ label_dst,
                                                       TI* __restrict__ inst_dst, const unsigned* __restrict__ protect,
                                                       unsigned char* __restrict__ changed, int* __restrict__ status,
                                                       LePlace p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int wx = tx * LE_TW + lane, wy = ty * LE_TH + wave;  // inside the clipped window
  const int x = p.cx0 + wx, y = p.cy0 + wy;
  bool hit = false;
  if (wx < p.cw && wy < p.chh) {
    const int u = xs[x - p.dx0], v = ys[y - p.dy0];
    hit = (unsigned)u < (unsigned)p.sw && (unsigned)v < (unsigned)p.sh &&
          le_is(inst_src[(size_t)(p.sy0 + v) * p.Ws + (p.sx0 + u)], p.id);
  }
  le_place_commit(hit, x, y, label_dst, inst_dst, protect, changed, status, p);
}

// The inverse affine map of include/him.h "Affine layout edits": six coefficients in units of 2^-24 source pixel, passed
// by value in the kernel arguments.
struct LeAffine {
  long long a00, a01, a02, a10, a11, a12;
};
#define AF_FRAC 24
#define AF_MAX_LIN (1ll << 30)
#define AF_MAX_OFF (1ll << 52)
#define AF_MAX_WIN 2048

// him_layout_place_affine's kernel: le_place_kernel with the two table reads replaced by the integer map; the nearest
// source pixel is floor((U + 2^23) / 2^24) (an arithmetic shift), compared against the source box in 64 bits.
template <typename TL, typename TI>
__global__ __launch_bounds__(256) void le_place_affine_kernel(const TI* __restrict__ inst_src, LeAffine m,
                                                              TL* __restrict__ label_dst, TI* __restrict__ inst_dst,
                                                              const unsigned* __restrict__ protect,
                                                              unsigned char* __restrict__ changed, int* __restrict__ status,
                                                              LePlace p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int wx = tx * LE_TW + lane, wy = ty * LE_TH + wave;  // inside the clipped window
  const int x = p.cx0 + wx, y = p.cy0 + wy;
  bool hit = false;
  if (wx < p.cw && wy < p.chh) {
    const long long u = ((m.a00 * x + m.a01 * y + m.a02 + (1ll << (AF_FRAC - 1))) >> AF_FRAC) - p.sx0;
    const long long v = ((m.a10 * x + m.a11 * y + m.a12 + (1ll << (AF_FRAC - 1))) >> AF_FRAC) - p.sy0;
    hit = u >= 0 && u < p.sw && v >= 0 && v < p.sh &&
          le_is(inst_src[(size_t)(p.sy0 + (int)v) * p.Ws + (p.sx0 + (int)u)], p.id);
  }
  le_place_commit(hit, x, y, label_dst, inst_dst, protect, changed, status, p);
}

// Keys' cubic convolution kernel, a = -0.5 (data/resample.py's BICUBIC), in fp64: w[0..3] at the distances 1 + t, t,
// 1 - t, 2 - t of the taps i - 1 .. i + 2.  t in [0, 1) is a multiple of 2^-24, exact; t == 0 gives exactly (0, 1, 0, 0).
__device__ __forceinline__ void af_keys(double t, double* w) {
  const double a = -0.5;
  const double d0 = 1.0 + t, d1 = t, d2 = 1.0 - t, d3 = 2.0 - t;
  w[0] = ((a * d0 - 5.0 * a) * d0 + 8.0 * a) * d0 - 4.0 * a;
  w[1] = ((a + 2.0) * d1 - (a + 3.0)) * d1 * d1 + 1.0;
  w[2] = ((a + 2.0) * d2 - (a + 3.0)) * d2 * d2 + 1.0;
  w[3] = ((a * d3 - 5.0 * a) * d3 + 8.0 * a) * d3 - 4.0 * a;
}

struct AfWarp {
  int Hs, Ws, x0, y0, H, W, tiles_x;
};

// him_canvas_warp_affine's kernel: the 64 x 4 tile of the place kernels, lane = column, the three channels in one thread.
// Sixteen clamped taps per channel gathered straight from global memory (a tile's source footprint is a few KB: L1 / L2),
// weights and the 48 multiply-adds in fp64, one narrowing to fp32 per output, plain stores.
__global__ __launch_bounds__(256) void af_warp_kernel(const float* __restrict__ src, LeAffine m, float* __restrict__ P,
                                                      AfWarp g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
  const int wx = tx * LE_TW + lane, wy = ty * LE_TH + wave;
  if (wx >= g.W || wy >= g.H) return;
  const long long x = (long long)g.x0 + wx, y = (long long)g.y0 + wy;
  const long long U = m.a00 * x + m.a01 * y + m.a02, V = m.a10 * x + m.a11 * y + m.a12;
  const long long ix = U >> AF_FRAC, iy = V >> AF_FRAC;
  const long long fmask = (1ll << AF_FRAC) - 1;
  double wxk[4], wyk[4];
  af_keys((double)(U & fmask) * (1.0 / (double)(1ll << AF_FRAC)), wxk);
  af_keys((double)(V & fmask) * (1.0 / (double)(1ll << AF_FRAC)), wyk);
  int cx[4], cy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long sx = ix - 1 + k, sy = iy - 1 + k;  // edge replicate, clamped in 64 bits before narrowing
    cx[k] = (int)(sx < 0 ? 0 : (sx > g.Ws - 1 ? g.Ws - 1 : sx));
    cy[k] = (int)(sy < 0 ? 0 : (sy > g.Hs - 1 ? g.Hs - 1 : sy));
  }
  const size_t plane = (size_t)g.Hs * g.Ws, out_plane = (size_t)g.H * g.W, o = (size_t)wy * g.W + wx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* __restrict__ s = src + c * plane;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* __restrict__ row = s + (size_t)cy[j] * g.Ws;
      double r = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) r += wxk[i] * (double)row[cx[i]];
      acc += wyk[j] * r;
    }
    P[c * out_plane + o] = (float)acc;
  }
}

static const int le_esize[4] = {1, 4, 8, 4};

static inline size_t le_up16(size_t n) { return (n + 15) / 16 * 16; }
static inline bool le_shape_ok(int H, int W) { return H >= 1 && W >= 1 && H <= LE_MAXDIM && W <= LE_MAXDIM; }
// can a plane of `kind` hold the id v exactly?
static inline bool le_fits(int kind, int v) {
  if (kind == 0) return v >= 0 && v <= 255;
  if (kind == 3) return v >= -(1 << 24) && v <= (1 << 24);
  return true;
}
static inline bool le_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}
static inline unsigned le_grid(long long n) {
  const long long blocks = (n + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

// the typed launches behind the untyped entry points
struct LeErase {
  const void *label, *inst;
  const unsigned char* region;
  int id;
  long long hw;
  const unsigned* fill;
  int n_class;
  unsigned char* seeds;
  const int *nearest, *edt_status;
  void *label_out, *inst_out;
  unsigned char* changed;
  int* status;
};

template <typename TL, typename TI>
static void le_launch_seed(const LeErase& e, hipStream_t st) {
  hipLaunchKernelGGL((le_seed_kernel<TL, TI>), dim3(le_grid(e.hw)), dim3(256), 0, st, (const TL*)e.label, (const TI*)e.inst,
                     e.region, e.id, e.hw, e.fill, e.n_class, e.seeds, (TL*)e.label_out, (TI*)e.inst_out, e.changed,
                     e.status);
}
template <typename TL, typename TI>
static void le_launch_gather(const LeErase& e, hipStream_t st) {
  hipLaunchKernelGGL((le_gather_kernel<TL, TI>), dim3(le_grid(e.hw)), dim3(256), 0, st, (const TL*)e.label,
                     (const TI*)e.inst, e.region, e.id, e.hw, e.n_class, e.nearest, e.edt_status, (TL*)e.label_out,
                     (TI*)e.inst_out, e.changed, e.status);
}

struct LePlaceArgs {
  const void* inst_src;
  const int *xs, *ys;
  void *label_dst, *inst_dst;
  const unsigned* protect;
  unsigned char* changed;
  int* status;
  LePlace p;
  LeAffine m;  // read by the affine launch only
};
template <typename TL, typename TI>
static void le_launch_place(const LePlaceArgs& a, hipStream_t st) {
  const int tiles_y = (a.p.chh + LE_TH - 1) / LE_TH;
  hipLaunchKernelGGL((le_place_kernel<TL, TI>), dim3((unsigned)(a.p.tiles_x * tiles_y)), dim3(256), 0, st,
                     (const TI*)a.inst_src, a.xs, a.ys, (TL*)a.label_dst, (TI*)a.inst_dst, a.protect, a.changed, a.status,
                     a.p);
}
template <typename TL, typename TI>
static void le_launch_place_affine(const LePlaceArgs& a, hipStream_t st) {
  const int tiles_y = (a.p.chh + LE_TH - 1) / LE_TH;
  hipLaunchKernelGGL((le_place_affine_kernel<TL, TI>), dim3((unsigned)(a.p.tiles_x * tiles_y)), dim3(256), 0, st,
                     (const TI*)a.inst_src, a.m, (TL*)a.label_dst, (TI*)a.inst_dst, a.protect, a.changed, a.status, a.p);
}

// the coefficients of an inverse map from the host array, refused beyond the limits of include/him.h
static bool af_load(const long long* inv, LeAffine* m) {
  const long long lim[6] = {AF_MAX_LIN, AF_MAX_LIN, AF_MAX_OFF, AF_MAX_LIN, AF_MAX_LIN, AF_MAX_OFF};
  for (int k = 0; k < 6; ++k)
    if (inv[k] > lim[k] || inv[k] < -lim[k]) return false;
  m->a00 = inv[0], m->a01 = inv[1], m->a02 = inv[2], m->a10 = inv[3], m->a11 = inv[4], m->a12 = inv[5];
  return true;
}

// FN<label type, instance type>(args, stream) for the two kinds
#define LE_BY_INST(FN, TL, ik, args, st)                  \
  switch (ik) {                                           \
    case 0: FN<TL, unsigned char>(args, st); break;       \
    case 1: FN<TL, int>(args, st); break;                 \
    case 2: FN<TL, long long>(args, st); break;           \
    default: FN<TL, float>(args, st); break;              \
  }
#define LE_BY_KINDS(FN, lk, ik, args, st)                             \
  switch (lk) {                                                       \
    case 0: LE_BY_INST(FN, unsigned char, ik, args, st) break;        \
    case 1: LE_BY_INST(FN, int, ik, args, st) break;                  \
    case 2: LE_BY_INST(FN, long long, ik, args, st) break;            \
    default: LE_BY_INST(FN, float, ik, args, st) break;               \
  }

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

// What both place entries are given besides their resampling operand (two device tables, or six host coefficients).
struct LePlaceCall {
  const void* inst_src;
  int inst_kind, Hs, Ws, id, sx0, sy0, sx1, sy1;
  void* label_dst;
  int label_kind;
  void* inst_dst;
  int Hd, Wd, dx0, dy0, dx1, dy1, cls, new_id;
  const unsigned int* protect;
  int n_class;
  unsigned char* changed;
  int* status;
};

// the argument checks both place entries share: HIM_OK, or the refusal
static int le_place_check(const char* what, const LePlaceCall& c) {
  if (!le_shape_ok(c.Hs, c.Ws) || !le_shape_ok(c.Hd, c.Wd))
    return fail(HIM_E_INVALID, "%s: bad shape (1 <= H, W <= %d)", what, LE_MAXDIM);
  if (c.label_kind < 0 || c.label_kind > 3 || c.inst_kind < 0 || c.inst_kind > 3)
    return fail(HIM_E_INVALID, "%s: kinds %d / %d", what, c.label_kind, c.inst_kind);
  if (c.sx0 < 0 || c.sy0 < 0 || c.sx1 <= c.sx0 || c.sy1 <= c.sy0 || c.sx1 > c.Ws || c.sy1 > c.Hs)
    return fail(HIM_E_INVALID, "%s: source box [%d, %d, %d, %d) is empty or not inside the %d x %d plane", what, c.sx0, c.sy0,
                c.sx1, c.sy1, c.Ws, c.Hs);
  if (c.dx1 <= c.dx0 || c.dy1 <= c.dy0 || c.dx0 < -LE_MAX_COORD || c.dy0 < -LE_MAX_COORD || c.dx1 > LE_MAX_COORD ||
      c.dy1 > LE_MAX_COORD)
    return fail(HIM_E_INVALID, "%s: destination box [%d, %d, %d, %d) is empty or beyond +-2^20", what, c.dx0, c.dy0, c.dx1,
                c.dy1);
  if (c.protect ? (c.n_class < 1 || c.n_class > LE_MAX_CLASS) : false)
    return fail(HIM_E_INVALID, "%s: n_class %d (1..%d)", what, c.n_class, LE_MAX_CLASS);
  if (!le_fits(c.label_kind, c.cls) || !le_fits(c.inst_kind, c.new_id))
    return fail(HIM_E_INVALID, "%s: class %d / id %d do not fit the planes' element types", what, c.cls, c.new_id);
  if (!c.inst_src || !c.label_dst || !c.inst_dst || !c.status) return fail(HIM_E_INVALID, "%s: null pointer", what);
  const int le = le_esize[c.label_kind], ie = le_esize[c.inst_kind];
  if ((uintptr_t)c.inst_src % ie != 0 || (uintptr_t)c.inst_dst % ie != 0 || (uintptr_t)c.label_dst % le != 0 ||
      (uintptr_t)c.protect % 4 != 0 || (uintptr_t)c.status % 4 != 0)
    return fail(HIM_E_INVALID, "%s: a pointer is not aligned to its element size", what);
  const size_t ns = (size_t)c.Hs * c.Ws * ie, nd = (size_t)c.Hd * c.Wd;
  if (le_overlap(c.inst_src, ns, c.label_dst, nd * le) || le_overlap(c.inst_src, ns, c.inst_dst, nd * ie) ||
      le_overlap(c.inst_src, ns, c.changed, nd))
    return fail(HIM_E_INVALID, "%s: the source plane overlaps a destination plane (place onto a copy)", what);
  if (le_overlap(c.label_dst, nd * le, c.inst_dst, nd * ie) || le_overlap(c.changed, nd, c.label_dst, nd * le) ||
      le_overlap(c.changed, nd, c.inst_dst, nd * ie))
    return fail(HIM_E_INVALID, "%s: two destination planes overlap", what);
  return HIM_OK;
}

// the launches both place entries share: the status init, the clipping, the tiling; `a` arrives with its resampling
// operand (xs / ys, or m) filled in by the entry
static int le_place_run(const char* what, const LePlaceCall& c, LePlaceArgs& a, bool affine, hipStream_t st) {
  hipLaunchKernelGGL(le_place_init_kernel, dim3(1), dim3(64), 0, st, c.status);
  const int cx0 = c.dx0 > 0 ? c.dx0 : 0, cy0 = c.dy0 > 0 ? c.dy0 : 0;
  const int cx1 = c.dx1 < c.Wd ? c.dx1 : c.Wd, cy1 = c.dy1 < c.Hd ? c.dy1 : c.Hd;
  if (cx1 > cx0 && cy1 > cy0) {
    a.inst_src = c.inst_src, a.label_dst = c.label_dst, a.inst_dst = c.inst_dst, a.protect = c.protect;
    a.changed = c.changed, a.status = c.status;
    a.p.Ws = c.Ws, a.p.id = c.id, a.p.sx0 = c.sx0, a.p.sy0 = c.sy0, a.p.sw = c.sx1 - c.sx0, a.p.sh = c.sy1 - c.sy0;
    a.p.Wd = c.Wd, a.p.dx0 = c.dx0, a.p.dy0 = c.dy0;
    a.p.cx0 = cx0, a.p.cy0 = cy0, a.p.cw = cx1 - cx0, a.p.chh = cy1 - cy0, a.p.tiles_x = (cx1 - cx0 + LE_TW - 1) / LE_TW;
    a.p.cls = c.cls, a.p.new_id = c.new_id, a.p.n_class = c.n_class;
    if (affine) {
      LE_BY_KINDS(le_launch_place_affine, c.label_kind, c.inst_kind, a, st)
    } else {
      LE_BY_KINDS(le_launch_place, c.label_kind, c.inst_kind, a, st)
    }
  }
  return check_launch(what);
}

extern "C" {

size_t him_layout_erase_workspace(int H, int W) {
  if (!le_shape_ok(H, W)) return 0;
  const size_t hw = (size_t)H * W;
  // seed plane, nearest, dist2, the job row + the transform's status, the transform's own workspace
  return le_up16(hw) + 2 * le_up16(hw * 4) + 32 + le_up16(him_edt_workspace(1, H, W));
}

int him_layout_erase(const void* label, int label_kind, const void* inst, int inst_kind, const unsigned char* region,
                     int id, int H, int W, const unsigned int* fill, int n_class, void* label_out, void* inst_out,
                     unsigned char* changed, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (!le_shape_ok(H, W)) return fail(HIM_E_INVALID, "layout_erase: bad shape (1 <= H, W <= %d)", LE_MAXDIM);
  if (label_kind < 0 || label_kind > 3 || inst_kind < 0 || inst_kind > 3)
    return fail(HIM_E_INVALID, "layout_erase: kinds %d / %d", label_kind, inst_kind);
  if (n_class < 1 || n_class > LE_MAX_CLASS) return fail(HIM_E_INVALID, "layout_erase: n_class %d (1..%d)", n_class, LE_MAX_CLASS);
  if (!label || !inst || !fill || !label_out || !inst_out || !changed || !status)
    return fail(HIM_E_INVALID, "layout_erase: null pointer");
  if (!ws) return fail(HIM_E_WORKSPACE, "layout_erase: null workspace");
  const int le = le_esize[label_kind], ie = le_esize[inst_kind];
  if ((uintptr_t)label % le != 0 || (uintptr_t)label_out % le != 0 || (uintptr_t)inst % ie != 0 ||
      (uintptr_t)inst_out % ie != 0 || (uintptr_t)fill % 4 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)ws % 16 != 0)
    return fail(HIM_E_INVALID, "layout_erase: a pointer is not aligned to its element size (ws: 16 bytes)");
  const size_t hw = (size_t)H * W;
  const void* outs[3] = {label_out, inst_out, changed};
  const size_t nout[3] = {hw * le, hw * ie, hw};
  const void* ins[3] = {label, inst, region};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b)
      if (le_overlap(outs[a], nout[a], ins[b], nout[b])) return fail(HIM_E_INVALID, "layout_erase: an output overlaps an input");
    for (int b = a + 1; b < 3; ++b)
      if (le_overlap(outs[a], nout[a], outs[b], nout[b])) return fail(HIM_E_INVALID, "layout_erase: two outputs overlap");
  }
  const size_t need = him_layout_erase_workspace(H, W);
  if (ws_bytes < need) return fail(HIM_E_WORKSPACE, "layout_erase: workspace %zu < %zu bytes", ws_bytes, need);
  unsigned char* seeds = (unsigned char*)ws;
  int* nearest = (int*)(seeds + le_up16(hw));
  int* dist2 = (int*)((unsigned char*)nearest + le_up16(hw * 4));
  int* jobs = (int*)((unsigned char*)dist2 + le_up16(hw * 4));
  int* edt_status = jobs + 4;
  unsigned char* edt_ws = (unsigned char*)jobs + 32;
  const LeErase e = {label, inst, region, id, (long long)hw, fill, n_class, seeds, nearest, edt_status, label_out, inst_out,
                     changed, status};
  hipLaunchKernelGGL(le_erase_init_kernel, dim3(1), dim3(64), 0, ST, jobs, status);
  LE_BY_KINDS(le_launch_seed, label_kind, inst_kind, e, ST)
  const int rc = him_edt(seeds, 0, 1, H, W, jobs, 1, dist2, nearest, edt_status, edt_ws, ws_bytes - (size_t)(edt_ws - seeds),
                         stream);
  if (rc != HIM_OK) return rc;
  LE_BY_KINDS(le_launch_gather, label_kind, inst_kind, e, ST)
  return check_launch("layout_erase");
}

int him_layout_place(const void* inst_src, int inst_kind, int Hs, int Ws, int id, int sx0, int sy0, int sx1, int sy1,
                     const int* xs, const int* ys, void* label_dst, int label_kind, void* inst_dst, int Hd, int Wd, int dx0,
                     int dy0, int dx1, int dy1, int cls, int new_id, const unsigned int* protect, int n_class,
                     unsigned char* changed, int* status, void* stream) {
  const char* what = "layout_place";
  const LePlaceCall c = {inst_src, inst_kind, Hs, Ws, id, sx0, sy0, sx1, sy1, label_dst, label_kind, inst_dst, Hd, Wd,
                         dx0, dy0, dx1, dy1, cls, new_id, protect, n_class, changed, status};
  const int rc = le_place_check(what, c);
  if (rc != HIM_OK) return rc;
  if (!xs || !ys) return fail(HIM_E_INVALID, "%s: null pointer", what);
  if ((uintptr_t)xs % 4 != 0 || (uintptr_t)ys % 4 != 0)
    return fail(HIM_E_INVALID, "%s: a pointer is not aligned to its element size", what);
  LePlaceArgs a;
  a.xs = xs, a.ys = ys;
  return le_place_run(what, c, a, false, ST);
}

int him_layout_place_affine(const void* inst_src, int inst_kind, int Hs, int Ws, int id, int sx0, int sy0, int sx1, int sy1,
                            const long long* inv, void* label_dst, int label_kind, void* inst_dst, int Hd, int Wd, int dx0,
                            int dy0, int dx1, int dy1, int cls, int new_id, const unsigned int* protect, int n_class,
                            unsigned char* changed, int* status, void* stream) {
  const char* what = "layout_place_affine";
  const LePlaceCall c = {inst_src, inst_kind, Hs, Ws, id, sx0, sy0, sx1, sy1, label_dst, label_kind, inst_dst, Hd, Wd,
                         dx0, dy0, dx1, dy1, cls, new_id, protect, n_class, changed, status};
  const int rc = le_place_check(what, c);
  if (rc != HIM_OK) return rc;
  if (!inv) return fail(HIM_E_INVALID, "%s: null pointer", what);
  if ((uintptr_t)inv % 8 != 0) return fail(HIM_E_INVALID, "%s: a pointer is not aligned to its element size", what);
  LePlaceArgs a;
  a.xs = a.ys = nullptr;
  if (!af_load(inv, &a.m))
    return fail(HIM_E_INVALID, "%s: a coefficient of the inverse map is beyond 2^30 (linear part) / 2^52 (offsets)", what);
  return le_place_run(what, c, a, true, ST);
}

int him_canvas_warp_affine(const float* src, int Hs, int Ws, const long long* inv, int x0, int y0, int H, int W, float* P,
                           void* stream) {
  if (!le_shape_ok(Hs, Ws)) return fail(HIM_E_INVALID, "canvas_warp_affine: source sides outside 1..%d", LE_MAXDIM);
  if (H < 1 || W < 1 || H > AF_MAX_WIN || W > AF_MAX_WIN)
    return fail(HIM_E_INVALID, "canvas_warp_affine: window %d x %d outside 1..%d per axis", W, H, AF_MAX_WIN);
  if (x0 < -LE_MAX_COORD || y0 < -LE_MAX_COORD || x0 > LE_MAX_COORD || y0 > LE_MAX_COORD)
    return fail(HIM_E_INVALID, "canvas_warp_affine: window origin (%d, %d) beyond +-2^20", x0, y0);
  if (!src || !inv || !P) return fail(HIM_E_INVALID, "canvas_warp_affine: null pointer");
  if ((uintptr_t)src % 4 != 0 || (uintptr_t)P % 4 != 0 || (uintptr_t)inv % 8 != 0)
    return fail(HIM_E_INVALID, "canvas_warp_affine: a pointer is not aligned to its element size");
  if (le_overlap(src, (size_t)3 * Hs * Ws * 4, P, (size_t)3 * H * W * 4))
    return fail(HIM_E_INVALID, "canvas_warp_affine: P overlaps src");
  LeAffine m;
  if (!af_load(inv, &m))
    return fail(HIM_E_INVALID, "canvas_warp_affine: a coefficient of the inverse map is beyond 2^30 (linear part) / 2^52 "
                               "(offsets)");
  AfWarp g;
  g.Hs = Hs, g.Ws = Ws, g.x0 = x0, g.y0 = y0, g.H = H, g.W = W, g.tiles_x = (W + LE_TW - 1) / LE_TW;
  const int tiles_y = (H + LE_TH - 1) / LE_TH;
  hipLaunchKernelGGL(af_warp_kernel, dim3((unsigned)(g.tiles_x * tiles_y)), dim3(256), 0, ST, src, m, P, g);
  return check_launch("canvas_warp_affine");
}

}  // extern "C"
