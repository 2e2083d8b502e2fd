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

template <typename TL, typename TI>
__global__ __launch_bounds__(256) void le_place_kernel(const TI* __restrict__ inst_src, const int* __restrict__ xs,
                                                       const int* __restrict__ ys, TL* __restrict__ label_dst,
                                                       TI* __restrict__ inst_dst, const unsigned* __restrict__ protect,
                                                       unsigned char* __restrict__ changed, int* __restrict__ status,
                                                       LePlace p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int wx = tx * LE_TW + lane, wy = ty * LE_TH + wave;  // inside the clipped window
  int wrote = 0, blocked = 0, x_lo = 0x7fffffff, y_lo = 0x7fffffff, x_hi = -1, y_hi = -1;
  if (wx < p.cw && wy < p.chh) {
    const int x = p.cx0 + wx, y = p.cy0 + wy;
    const int u = xs[x - p.dx0], v = ys[y - p.dy0];
    if ((unsigned)u < (unsigned)p.sw && (unsigned)v < (unsigned)p.sh &&
        le_is(inst_src[(size_t)(p.sy0 + v) * p.Ws + (p.sx0 + u)], p.id)) {
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
  }
  const int n_w = wave_sum_i32(wrote), n_b = wave_sum_i32(blocked);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x_lo = min(x_lo, __shfl_xor(x_lo, o, 64));
    y_lo = min(y_lo, __shfl_xor(y_lo, o, 64));
    x_hi = max(x_hi, __shfl_xor(x_hi, o, 64));
    y_hi = max(y_hi, __shfl_xor(y_hi, o, 64));
  }
  if (lane == 0) {
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
};
template <typename TL, typename TI>
static void le_launch_place(const LePlaceArgs& a, hipStream_t st) {
  const int tiles_y = (a.p.chh + LE_TH - 1) / LE_TH;
  hipLaunchKernelGGL((le_place_kernel<TL, TI>), dim3((unsigned)(a.p.tiles_x * tiles_y)), dim3(256), 0, st,
                     (const TI*)a.inst_src, a.xs, a.ys, (TL*)a.label_dst, (TI*)a.inst_dst, a.protect, a.changed, a.status,
                     a.p);
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
  if (!le_shape_ok(Hs, Ws) || !le_shape_ok(Hd, Wd))
    return fail(HIM_E_INVALID, "layout_place: bad shape (1 <= H, W <= %d)", LE_MAXDIM);
  if (label_kind < 0 || label_kind > 3 || inst_kind < 0 || inst_kind > 3)
    return fail(HIM_E_INVALID, "layout_place: kinds %d / %d", label_kind, inst_kind);
  if (sx0 < 0 || sy0 < 0 || sx1 <= sx0 || sy1 <= sy0 || sx1 > Ws || sy1 > Hs)
    return fail(HIM_E_INVALID, "layout_place: source box [%d, %d, %d, %d) is empty or not inside the %d x %d plane", sx0, sy0,
                sx1, sy1, Ws, Hs);
  if (dx1 <= dx0 || dy1 <= dy0 || dx0 < -LE_MAX_COORD || dy0 < -LE_MAX_COORD || dx1 > LE_MAX_COORD || dy1 > LE_MAX_COORD)
    return fail(HIM_E_INVALID, "layout_place: destination box [%d, %d, %d, %d) is empty or beyond +-2^20", dx0, dy0, dx1, dy1);
  if (protect ? (n_class < 1 || n_class > LE_MAX_CLASS) : false)
    return fail(HIM_E_INVALID, "layout_place: n_class %d (1..%d)", n_class, LE_MAX_CLASS);
  if (!le_fits(label_kind, cls) || !le_fits(inst_kind, new_id))
    return fail(HIM_E_INVALID, "layout_place: class %d / id %d do not fit the planes' element types", cls, new_id);
  if (!inst_src || !xs || !ys || !label_dst || !inst_dst || !status) return fail(HIM_E_INVALID, "layout_place: null pointer");
  const int le = le_esize[label_kind], ie = le_esize[inst_kind];
  if ((uintptr_t)inst_src % ie != 0 || (uintptr_t)inst_dst % ie != 0 || (uintptr_t)label_dst % le != 0 ||
      (uintptr_t)xs % 4 != 0 || (uintptr_t)ys % 4 != 0 || (uintptr_t)protect % 4 != 0 || (uintptr_t)status % 4 != 0)
    return fail(HIM_E_INVALID, "layout_place: a pointer is not aligned to its element size");
  const size_t ns = (size_t)Hs * Ws * ie, nd = (size_t)Hd * Wd;
  if (le_overlap(inst_src, ns, label_dst, nd * le) || le_overlap(inst_src, ns, inst_dst, nd * ie) ||
      le_overlap(inst_src, ns, changed, nd))
    return fail(HIM_E_INVALID, "layout_place: the source plane overlaps a destination plane (place onto a copy)");
  if (le_overlap(label_dst, nd * le, inst_dst, nd * ie) || le_overlap(changed, nd, label_dst, nd * le) ||
      le_overlap(changed, nd, inst_dst, nd * ie))
    return fail(HIM_E_INVALID, "layout_place: two destination planes overlap");
  hipLaunchKernelGGL(le_place_init_kernel, dim3(1), dim3(64), 0, ST, status);
  const int cx0 = dx0 > 0 ? dx0 : 0, cy0 = dy0 > 0 ? dy0 : 0;
  const int cx1 = dx1 < Wd ? dx1 : Wd, cy1 = dy1 < Hd ? dy1 : Hd;
  if (cx1 > cx0 && cy1 > cy0) {
    LePlaceArgs a;
    a.inst_src = inst_src, a.xs = xs, a.ys = ys, a.label_dst = label_dst, a.inst_dst = inst_dst, a.protect = protect;
    a.changed = changed, a.status = status;
    a.p.Ws = Ws, a.p.id = id, a.p.sx0 = sx0, a.p.sy0 = sy0, a.p.sw = sx1 - sx0, a.p.sh = sy1 - sy0;
    a.p.Wd = Wd, a.p.dx0 = dx0, a.p.dy0 = dy0;
    a.p.cx0 = cx0, a.p.cy0 = cy0, a.p.cw = cx1 - cx0, a.p.chh = cy1 - cy0, a.p.tiles_x = (cx1 - cx0 + LE_TW - 1) / LE_TW;
    a.p.cls = cls, a.p.new_id = new_id, a.p.n_class = n_class;
    LE_BY_KINDS(le_launch_place, label_kind, inst_kind, a, ST)
  }
  return check_launch("layout_place");
}

}  // extern "C"
