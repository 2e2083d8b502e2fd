// Connected-component instance labelling of class planes (include/him.h "Instance labelling of layouts"): a union-find
// labelling in seven plain launches on one stream.  No cooperative launch, no grid-wide barrier, and no workgroup ever
// waits for another one.
//
//   1 tile    a 256-thread workgroup owns CCL_TH x CCL_TW = 32 x 64 pixels; lane = column, a wave = one tile row, so
//             every row-wise LDS access is 64 consecutive dwords (conflict-free) and the runs of a row come from ONE
//             ballot.  Runs are then joined upwards (and diagonally) by atomicMin on an int32 parent per pixel in LDS,
//             the tile is flattened and the parents leave as plane-linear indices (-1: the pixel has no instances).
//   2 border  every pixel of a tile's top row / left column joins its neighbours in the adjacent tiles: atomicMin on
//             the global parents.
//   3 flatten parent := root; a root's area is counted with integer atomicAdd, one add per distinct root of a wave.
//   4 count   kept roots (root of itself, area >= min_area) per chunk of CCL_CHUNK pixels,
//   5 scan    one workgroup per plane: exclusive prefix sum of the chunk counts, and the plane's status record,
//   6 rank    a kept root's rank = chunk offset + its position among the chunk's kept roots, stored in its area cell,
//   7 write   inst_out = base_id + rank of the pixel's root, or the pixel's class.
//
// TERMINATION.  A parent is only ever lowered (atomicMin, or a store of a root that lies below it) and parent[x] <= x
// always.  A `find` follows strictly decreasing indices and stops at the first cell that holds its own index.  A union
// goes round again only with one of its two indices replaced by a strictly smaller one (the value the atomicMin found
// in the cell), so the sum of the two falls every round.  Neither loop needs any other thread to make progress.
//
// DETERMINISM.  Links always point from a higher index to a lower one of the same component, and a union never drops a
// link without re-joining what it pointed to.  The smallest index m of a component can point nowhere but to itself, so
// it is a root, and once all unions are done a component has exactly one root: m, whatever the order of the atomics.
// A read that sees an older value of a cell sees an ancestor all the same.  Areas are integer sums, ranks come from a
// prefix sum in raster order and not from a counter: inst_out and status are bit-identical from run to run.
#include "him_common.h"

namespace him {

#define CCL_TH 32
#define CCL_TW 64
#define CCL_TPX (CCL_TH * CCL_TW)
#define CCL_ROWS (CCL_TH / 4)         // tile rows per thread: wave w owns the rows w, w + 4, ...
#define CCL_CHUNK 2048                // pixels per workgroup of the count / rank passes
#define CCL_PER (CCL_CHUNK / 256)
#define CCL_MAX_BLOCKS (1 << 20)      // grid cap of the strided loops
#define CCL_MAX_PIXELS (1LL << 40)    // B * H * W; keeps every byte count far inside size_t

// class of a pixel, -2: outside 0..255 (or a non-integral fp32)
__device__ __forceinline__ int ccl_cls(unsigned char v) { return (int)v; }
__device__ __forceinline__ int ccl_cls(int v) { return (v >= 0 && v < 256) ? v : -2; }
__device__ __forceinline__ int ccl_cls(long long v) { return (v >= 0 && v < 256) ? (int)v : -2; }
__device__ __forceinline__ int ccl_cls(float v) { return (v >= 0.0f && v < 256.0f && v == floorf(v)) ? (int)v : -2; }

__device__ __forceinline__ int ccl_lds_find(int* P, int x) {
  int p;
  while ((p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;  // p < x: see TERMINATION
  return x;
}
__device__ __forceinline__ void ccl_lds_union(int* P, int a, int b) {
  for (;;) {
    a = ccl_lds_find(P, a);
    b = ccl_lds_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[a], b);
    if (old == a) return;      // a was still a root: it now hangs under b
    a = old;                   // old < a: whatever a pointed to still has to meet b (see TERMINATION)
  }
}

__device__ __forceinline__ int ccl_find(int* P, int x) {
  int p;
  while ((p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;      // p < x
  return x;
}
__device__ __forceinline__ void ccl_union(int* P, int a, int b) {
  for (;;) {
    a = ccl_find(P, a);
    b = ccl_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[a], b);
    if (old == a) return;
    a = old;                   // old < a, as in ccl_lds_union
  }
}

// ---- 1: tile pass.  parent / area of every pixel of the plane are written here, so the workspace needs no clearing.
template <typename T>
__global__ __launch_bounds__(256) void ccl_tile_kernel(const T* __restrict__ cls, int H, int W, int tilesX, int tilesPer,
                                                       long long tiles, const unsigned char* __restrict__ thing,
                                                       int conn8, int* __restrict__ parent, int* __restrict__ area,
                                                       int* __restrict__ tileflag) {
  __shared__ int P[CCL_TPX];
  __shared__ short C[CCL_TPX];          // class of a pixel that has instances, else -1
  __shared__ unsigned char TH[256];
  const int col = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const long long HW = (long long)H * W;
  TH[threadIdx.x] = thing[threadIdx.x];
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();
    const int b = (int)(t / tilesPer), tp = (int)(t - (long long)b * tilesPer);
    const int y0 = (tp / tilesX) * CCL_TH, x0 = (tp % tilesX) * CCL_TW;
    const T* plane = cls + (long long)b * HW;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < CCL_ROWS; ++k) {
      const int row = r0 + 4 * k, y = y0 + row, x = x0 + col;
      int tc = -1;
      if (y < H && x < W) {
        const int c = ccl_cls(plane[(long long)y * W + x]);
        if (c < 0) bad = 1;
        else if (TH[c]) tc = c;
      }
      C[row * CCL_TW + col] = (short)tc;
    }
    __syncthreads();
    // the runs of a row: a wave holds the whole row, the start of a lane's run is the highest start bit at or below it
#pragma unroll
    for (int k = 0; k < CCL_ROWS; ++k) {
      const int l = (r0 + 4 * k) * CCL_TW + col;
      const int start = (col == 0 || C[l - 1] != C[l]) ? 1 : 0;
      const unsigned long long starts = __ballot(start);
      const unsigned long long le = col == 63 ? ~0ull : ((1ull << (col + 1)) - 1ull);
      P[l] = l - col + (63 - __clzll((long long)(starts & le)));
    }
    __syncthreads();
    // join runs upwards.  A pixel whose left neighbour lies in the same run AND under the same upper run leaves the
    // union to that neighbour; with 8-connectivity the diagonals matter only where the pixel above is of another class
    // (else they lie in its run), and the up-left one only at the start of a run (else the left neighbour has it above).
#pragma unroll
    for (int k = 0; k < CCL_ROWS; ++k) {
      const int row = r0 + 4 * k, l = row * CCL_TW + col;
      const int tc = C[l];
      if (tc < 0 || row == 0) continue;
      const int up = C[l - CCL_TW];
      const int lf = col > 0 ? C[l - 1] : -2, ul = col > 0 ? C[l - CCL_TW - 1] : -2;
      if (up == tc) {
        if (!(lf == tc && ul == tc)) ccl_lds_union(P, l, l - CCL_TW);
      } else if (conn8) {
        if (ul == tc && lf != tc) ccl_lds_union(P, l, l - CCL_TW - 1);
        if (col < 63 && C[l - CCL_TW + 1] == tc) ccl_lds_union(P, l, l - CCL_TW + 1);
      }
    }
    __syncthreads();
    // tile raster order is plane raster order restricted to the tile: the tile's minimum is the plane's minimum of it
#pragma unroll
    for (int k = 0; k < CCL_ROWS; ++k) {
      const int row = r0 + 4 * k, y = y0 + row, x = x0 + col, l = row * CCL_TW + col;
      if (y < H && x < W) {
        int g = -1;
        if (C[l] >= 0) {
          const int root = ccl_lds_find(P, l);
          g = (y0 + (root >> 6)) * W + x0 + (root & 63);
        }
        const long long at = (long long)b * HW + (long long)y * W + x;
        parent[at] = g;
        area[at] = 0;
      }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) tileflag[t] = bad ? HIM_CCL_CLS_RANGE : 0;
  }
}

template <typename T>
__device__ __forceinline__ int ccl_thing_class(const T* __restrict__ plane, long long at,
                                               const unsigned char* __restrict__ thing) {
  const int c = ccl_cls(plane[at]);
  return (c >= 0 && thing[c]) ? c : -1;
}

// ---- 2: border pass.  Items of a plane: (tilesY - 1) * W pixels on top rows of tiles, then (tilesX - 1) * H pixels on
// left columns.  A top-row pixel looks up (and up-left / up-right), a left-column pixel looks left (and up-left /
// down-left): every pair of 8-neighbours in different tiles has its lower pixel on a top row or its right pixel on a
// left column.  The neighbour coordinates are checked against the plane, the own ones lie inside it by construction.
template <typename T>
__global__ __launch_bounds__(256) void ccl_border_kernel(const T* __restrict__ cls, int H, int W, int tilesX, int tilesY,
                                                         int B, const unsigned char* __restrict__ thing, int conn8,
                                                         int* parent) {
  const long long HW = (long long)H * W;
  const long long nh = (long long)(tilesY - 1) * W, per = nh + (long long)(tilesX - 1) * H, total = per * B;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int b = (int)(i / per);
    long long j = i - (long long)b * per;
    const bool top = j < nh;
    int y, x;
    if (top) {
      y = (int)(j / W + 1) * CCL_TH, x = (int)(j % W);
    } else {
      j -= nh;
      x = (int)(j / H + 1) * CCL_TW, y = (int)(j % H);
    }
    const T* plane = cls + (long long)b * HW;
    int* P = parent + (long long)b * HW;
    const int me = y * W + x;
    const int tc = ccl_thing_class(plane, me, thing);
    if (tc < 0) continue;
    if (top) {
      if (ccl_thing_class(plane, me - W, thing) == tc) ccl_union(P, me, me - W);
      if (conn8) {
        if (x > 0 && ccl_thing_class(plane, me - W - 1, thing) == tc) ccl_union(P, me, me - W - 1);
        if (x < W - 1 && ccl_thing_class(plane, me - W + 1, thing) == tc) ccl_union(P, me, me - W + 1);
      }
    } else {
      if (ccl_thing_class(plane, me - 1, thing) == tc) ccl_union(P, me, me - 1);
      if (conn8) {
        if (y > 0 && ccl_thing_class(plane, me - W - 1, thing) == tc) ccl_union(P, me, me - W - 1);
        if (y < H - 1 && ccl_thing_class(plane, (long long)me + W - 1, thing) == tc) ccl_union(P, me, me + W - 1);
      }
    }
  }
}

// ---- 3: flatten.  No union runs any more; a cell another thread overwrites meanwhile goes from an ancestor to the root,
// and either serves the walk.  The lanes of a wave that found the same root add their number once.
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int* parent, int* __restrict__ area, long long total,
                                                          long long HW) {
  const int lane = threadIdx.x & 63;
  for (long long base = blockIdx.x * 256LL; base < total; base += gridDim.x * 256LL) {
    const long long i = base + threadIdx.x;
    int root = -1, b = 0;
    if (i < total) {
      b = (int)(i / HW);
      const int first = parent[i];
      if (first >= 0) {
        const int* P = parent + (long long)b * HW;
        int x = first, p;
        while ((p = P[x]) != x) x = p;      // p < x
        root = x;
        if (root != first) parent[i] = root;
      }
    }
    unsigned long long todo = __ballot(root >= 0);
    while (todo) {                           // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lr = __shfl(root, leader, 64), lb = __shfl(b, leader, 64);
      const unsigned long long same = __ballot(root == lr && b == lb);
      if (lane == leader) atomicAdd(&area[(long long)lb * HW + lr], __popcll(same));
      todo &= ~same;
    }
  }
}

__device__ __forceinline__ int ccl_kept(const int* __restrict__ parent, const int* __restrict__ area, long long pb,
                                        long long li, long long HW, int min_area) {
  return (li < HW && parent[pb + li] == (int)li && area[pb + li] >= min_area) ? 1 : 0;
}

// ---- 4: kept roots per chunk of CCL_CHUNK pixels (chunk c = plane c / G, pixels (c % G) * CCL_CHUNK ...)
__global__ __launch_bounds__(256) void ccl_count_kernel(const int* __restrict__ parent, const int* __restrict__ area,
                                                        long long HW, int G, long long chunks, int min_area,
                                                        int* __restrict__ bcount) {
  __shared__ int sh[4];
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    const long long b = c / G, pb = b * HW, l0 = (c - b * G) * CCL_CHUNK;
    int n = 0;
#pragma unroll
    for (int k = 0; k < CCL_PER; ++k) n += ccl_kept(parent, area, pb, l0 + k * 256 + threadIdx.x, HW, min_area);
    n = block_sum_i32(n, sh);
    if (threadIdx.x == 0) bcount[c] = n;
  }
}

// ---- 5: one workgroup per plane: bcount := its exclusive prefix sum, status := count and flags
__global__ __launch_bounds__(256) void ccl_scan_kernel(int* __restrict__ bcount, const int* __restrict__ tileflag, int G,
                                                       int tilesPer, int max_objects, int base_id,
                                                       int* __restrict__ status) {
  __shared__ int sh[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long b = blockIdx.x;
  int* bc = bcount + b * G;
  int carry = 0;
  for (int g0 = 0; g0 < G; g0 += 256) {
    const int g = g0 + threadIdx.x;
    const int v = g < G ? bc[g] : 0;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    __syncthreads();
    if (lane == 63) sh[w] = s;
    __syncthreads();
    int below = 0;
    for (int j = 0; j < w; ++j) below += sh[j];
    if (g < G) bc[g] = carry + below + s - v;
    carry += (sh[0] + sh[1]) + (sh[2] + sh[3]);
  }
  int f = 0;
  for (int t = threadIdx.x; t < tilesPer; t += 256) f |= tileflag[b * tilesPer + t];
  f = __syncthreads_or(f);
  if (threadIdx.x == 0) {
    int flags = f ? HIM_CCL_CLS_RANGE : 0;
    if (carry > max_objects || (long long)base_id + carry - 1 > 65535) flags |= HIM_CCL_OVERFLOW;
    status[2 * b] = carry;
    status[2 * b + 1] = flags;
  }
}

// ---- 6: a root's area cell := its rank among the plane's kept roots in raster order, -1 for a root that is dropped.
// Only the thread that owns pixel i reads or writes area[i] here.
__global__ __launch_bounds__(256) void ccl_rank_kernel(const int* __restrict__ parent, int* __restrict__ area,
                                                       long long HW, int G, long long chunks, int min_area,
                                                       const int* __restrict__ bcount) {
  __shared__ int sh[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    const long long b = c / G, pb = b * HW, l0 = (c - b * G) * CCL_CHUNK;
    int carry = bcount[c];
#pragma unroll 1
    for (int k = 0; k < CCL_PER; ++k) {
      const long long li = l0 + k * 256 + threadIdx.x;
      const bool root = li < HW && parent[pb + li] == (int)li;
      const int keep = ccl_kept(parent, area, pb, li, HW, min_area);
      const unsigned long long votes = __ballot(keep);
      __syncthreads();
      if (lane == 0) sh[w] = __popcll(votes);
      __syncthreads();
      int below = 0;
      for (int j = 0; j < w; ++j) below += sh[j];
      if (root) area[pb + li] = keep ? carry + below + __popcll(votes & ((1ull << lane) - 1ull)) : -1;
      carry += (sh[0] + sh[1]) + (sh[2] + sh[3]);
    }
  }
}

// ---- 7: the instance plane
template <typename T>
__global__ __launch_bounds__(256) void ccl_write_kernel(const T* __restrict__ cls, const int* __restrict__ parent,
                                                        const int* __restrict__ area, long long total, long long HW,
                                                        int base_id, int* __restrict__ out) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int p = parent[i];
    int v = ccl_cls(cls[i]);
    if (p >= 0) {
      const int r = area[i / HW * HW + p];
      if (r >= 0) v = base_id + r;
    }
    out[i] = v;
  }
}

static inline long long ccl_div(long long a, long long b) { return (a + b - 1) / b; }
static inline dim3 ccl_grid(long long blocks) {
  return dim3((unsigned)(blocks < 1 ? 1 : (blocks > CCL_MAX_BLOCKS ? CCL_MAX_BLOCKS : blocks)));
}
// "" when the shape is served, else why not
static inline const char* ccl_shape_error(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return "B, H and W must be at least 1";
  if ((long long)H * W > 0x7fffffffLL) return "H * W exceeds 2^31 - 1";
  if ((long long)B * ((long long)H * W) > CCL_MAX_PIXELS) return "B * H * W exceeds 2^40";
  return "";
}
static inline size_t ccl_ws_bytes(int B, int H, int W) {
  const long long HW = (long long)H * W;
  const long long ints = 2 * (B * HW) + B * ccl_div(HW, CCL_CHUNK) + B * (ccl_div(H, CCL_TH) * ccl_div(W, CCL_TW));
  return ((size_t)ints * sizeof(int) + 15) / 16 * 16;
}

template <typename T>
static void ccl_launch(const T* cls, int B, int H, int W, const unsigned char* thing, int conn8, int min_area,
                       int base_id, int max_objects, int* inst_out, int* status, int* ws, hipStream_t st) {
  const long long HW = (long long)H * W, total = B * HW;
  const int tilesX = (int)ccl_div(W, CCL_TW), tilesY = (int)ccl_div(H, CCL_TH), tilesPer = tilesX * tilesY;
  const int G = (int)ccl_div(HW, CCL_CHUNK);
  const long long tiles = (long long)B * tilesPer, chunks = (long long)B * G;
  int* parent = ws;
  int* area = parent + total;
  int* bcount = area + total;
  int* tileflag = bcount + chunks;
  hipLaunchKernelGGL(ccl_tile_kernel<T>, ccl_grid(tiles), dim3(256), 0, st, cls, H, W, tilesX, tilesPer, tiles, thing,
                     conn8, parent, area, tileflag);
  const long long items = B * ((long long)(tilesY - 1) * W + (long long)(tilesX - 1) * H);
  if (items > 0)
    hipLaunchKernelGGL(ccl_border_kernel<T>, ccl_grid(ccl_div(items, 256)), dim3(256), 0, st, cls, H, W, tilesX, tilesY,
                       B, thing, conn8, parent);
  hipLaunchKernelGGL(ccl_flatten_kernel, ccl_grid(ccl_div(total, 256)), dim3(256), 0, st, parent, area, total, HW);
  hipLaunchKernelGGL(ccl_count_kernel, ccl_grid(chunks), dim3(256), 0, st, parent, area, HW, G, chunks, min_area, bcount);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, bcount, tileflag, G, tilesPer, max_objects,
                     base_id, status);
  hipLaunchKernelGGL(ccl_rank_kernel, ccl_grid(chunks), dim3(256), 0, st, parent, area, HW, G, chunks, min_area, bcount);
  hipLaunchKernelGGL(ccl_write_kernel<T>, ccl_grid(ccl_div(total, 256)), dim3(256), 0, st, cls, parent, area, total, HW,
                     base_id, inst_out);
}

}  // namespace him

using namespace him;

extern "C" {

size_t him_label_instances_workspace(int B, int H, int W) {
  if (ccl_shape_error(B, H, W)[0]) return 0;
  return ccl_ws_bytes(B, H, W);
}

int him_label_instances(const void* cls, int cls_kind, int B, int H, int W, const unsigned char* thing, int connectivity,
                        int min_area, int base_id, int max_objects, int* inst_out, int* status, void* ws,
                        size_t ws_bytes, void* stream) {
  const char* why = ccl_shape_error(B, H, W);
  if (why[0]) return fail(HIM_E_INVALID, "label_instances: %s (B %d, H %d, W %d)", why, B, H, W);
  if (!cls || !thing || !inst_out || !status || !ws) return fail(HIM_E_INVALID, "label_instances: null pointer");
  if (cls_kind < 0 || cls_kind > 3) return fail(HIM_E_INVALID, "label_instances: cls_kind %d", cls_kind);
  if (connectivity != 4 && connectivity != 8)
    return fail(HIM_E_INVALID, "label_instances: connectivity %d (4 or 8)", connectivity);
  if (base_id < 256) return fail(HIM_E_INVALID, "label_instances: base_id %d (at least 256)", base_id);
  if (max_objects < 1 || max_objects > 65536)
    return fail(HIM_E_INVALID, "label_instances: max_objects %d (1..65536)", max_objects);
  if ((uintptr_t)ws % 16 != 0) return fail(HIM_E_INVALID, "label_instances: workspace not 16-byte aligned");
  if (ws_bytes < ccl_ws_bytes(B, H, W))
    return fail(HIM_E_WORKSPACE, "label_instances: workspace %zu < %zu bytes", ws_bytes, ccl_ws_bytes(B, H, W));
  hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8 ? 1 : 0;
  switch (cls_kind) {
    case 0: ccl_launch((const unsigned char*)cls, B, H, W, thing, conn8, min_area, base_id, max_objects, inst_out, status,
                       (int*)ws, st); break;
    case 1: ccl_launch((const int*)cls, B, H, W, thing, conn8, min_area, base_id, max_objects, inst_out, status, (int*)ws,
                       st); break;
    case 2: ccl_launch((const long long*)cls, B, H, W, thing, conn8, min_area, base_id, max_objects, inst_out, status,
                       (int*)ws, st); break;
    default: ccl_launch((const float*)cls, B, H, W, thing, conn8, min_area, base_id, max_objects, inst_out, status,
                        (int*)ws, st); break;
  }
  return check_launch("label_instances");
}

}  // extern "C"
