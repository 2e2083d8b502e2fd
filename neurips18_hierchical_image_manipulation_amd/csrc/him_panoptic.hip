// Panoptic matching of layouts on the device (include/him.h "Panoptic matching"): per plane the segments of a predicted
// and a ground-truth (segment id, class) pair of planes, their pixel overlaps, the unique matches at IoU > 0.5 and the
// per-class tp / fp / fn counts and IoU sums behind panoptic quality (Kirillov et al., CVPR 2019).  All counting is in
// integers; the only floating-point work is one division per matched pair and their sum in a fixed order.
//
// Uniqueness of a match.  g holds no void pixel, so with p' = p \ void the union above is |g u p'| and inter = |g n p'|.
// 2 inter > |g u p'| >= max(|g|, |p'|): more than half of g lies in p and more than half of p' lies in g.  Segments of
// one side are disjoint, and two disjoint sets cannot both hold more than half of a third: a g has at most one p, a p at
// most one g.
//
// Seven launches on the caller's stream, no host synchronisation, no cooperative launch, no workgroup waits for another:
//   clear     the header (flags, counts) and the per-(plane, side) area tables of 65536 ids.
//   segment   workgroup (x, b) walks its share of the plane in steps of PQ_STEP = 256 lanes x PQ_PX = 4 pixels; a lane
//             reads its 4 pixels of every plane with one vector load where the bases are 16-byte aligned and W % 4 == 0,
//             else element by element.  It keeps ONE open run per side in registers (id, pixel count) across its steps --
//             the lane's pixels of consecutive steps lie PQ_STEP pixels apart, below one another in a layout -- and
//             issues one integer atomic add into the area table when the id changes.  The runs still open at the end are
//             merged over the wave when the whole wave holds one id (one atomic per wave: a plane of one id costs one
//             atomic per wave and share, not per lane).  Range checks of ids and classes set the plane's flags here.
//   rank      one 1024-thread workgroup per (plane, side): every thread holds 64 consecutive table entries in registers,
//             an exclusive prefix sum of "area > 0" gives the dense rank of every present id in ascending id
//             (np.unique's order); it writes the rank table, the id and area lists and the true count.
//   clear     the (n_gt + 1) x n_pred pair table of the plane (row 0 is void, row stride n_pred: only what the plane needs
//             is cleared and touched) and the per-segment class and matched arrays.
//   pair      the segment pass's walk with the key (ground-truth row, predicted rank); a lane looks a rank up only when
//             the id changes.  One int32 atomic add per run into the pair table, and integer atomic max of 256 - class
//             and class + 1 into the per-segment class arrays (so that zero means "nothing yet").
//   match     one wave per ground-truth row scans the predicted columns with inter > 0 for the class-equal column with
//             2 inter > union; it records the pair and marks the column (one writer: the match is unique).
//   reduce    one wave per class walks the planes and segments in a fixed order, lane l taking segments l, l + 64, ...,
//             and adds the lanes with the xor butterfly of him_common.h; one workgroup per plane writes the status row.
// Only integer atomics (add, max, or) are used: they commute, so every table is exact and every output is bit-identical
// from run to run.  A plane with HIM_PQ_OVERFLOW, HIM_PQ_ID_RANGE or HIM_PQ_CLS_RANGE is left by the pair, match and
// reduce passes before they index anything by a rank.
#include "him_common.h"

namespace him {

#define PQ_PX 4          // pixels per lane and step (the vector width of the aligned path)
#define PQ_IDS 65536     // the id domain
#define PQ_RANK_T 1024   // threads of the rank pass, PQ_IDS / PQ_RANK_T = 64 entries each
#define PQ_REFUSED (HIM_PQ_OVERFLOW | HIM_PQ_ID_RANGE | HIM_PQ_CLS_RANGE)
#define PQ_BAD (-(1LL << 62))   // a non-integral or far out of range fp32 value

struct PqLayout {
  size_t hdr, area, rank, seg, aux, res, pair, total;
  size_t ms, pair_stride;   // padded max_segments; ints per plane of the pair table
};

static inline PqLayout pq_layout(int B, int M) {
  PqLayout l;
  l.ms = ((size_t)M + 3) & ~(size_t)3;
  l.pair_stride = (((size_t)M + 1) * (size_t)M + 3) & ~(size_t)3;
  size_t o = 0;
  l.hdr = o, o += (size_t)B * 16;
  l.area = o, o += (size_t)B * 2 * PQ_IDS * 4;
  l.rank = o, o += (size_t)B * 2 * PQ_IDS * 4;
  l.seg = o, o += (size_t)B * 4 * l.ms * 4;    // [b][side][id | area][ms]
  l.aux = o, o += (size_t)B * 5 * l.ms * 4;    // [b][gt 256-cls max | gt cls+1 max | pred ... | pred ... | matched][ms]
  l.res = o, o += (size_t)B * 3 * l.ms * 4;    // [b][matched rank | inter | union][ms]
  l.pair = o, o += (size_t)B * l.pair_stride * 4;
  l.total = o;
  return l;
}

struct PqPlanes {
  const void* pseg;
  const void* pcls;
  const void* gseg;
  const void* gcls;
  const float* mask;
  int pseg_kind, pcls_kind, gseg_kind, gcls_kind;
};

// 4 values of plane element i0.. as 64-bit integers.  kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 (PQ_BAD unless integral
// and within +-2^31).  vec: one aligned vector load; else element by element, 0 behind the plane's end.
__device__ __forceinline__ long long pq_f32(float v) {
  return (v >= -2147483648.0f && v < 2147483648.0f && v == floorf(v)) ? (long long)v : PQ_BAD;
}
__device__ __forceinline__ void pq_load4(const void* __restrict__ plane, int kind, long long i0, long long n, bool vec,
                                         long long v[PQ_PX]) {
  switch (kind) {
    case 0: {
      const unsigned char* p = (const unsigned char*)plane;
      if (vec) {
        const unsigned q = *(const unsigned*)(p + i0);
#pragma unroll
        for (int k = 0; k < PQ_PX; ++k) v[k] = (long long)((q >> (8 * k)) & 255u);
      } else {
#pragma unroll
        for (int k = 0; k < PQ_PX; ++k) v[k] = i0 + k < n ? (long long)p[i0 + k] : 0;
      }
      break;
    }
    case 1: {
      const int* p = (const int*)plane;
      if (vec) {
        const int4 q = *(const int4*)(p + i0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < PQ_PX; ++k) v[k] = i0 + k < n ? (long long)p[i0 + k] : 0;
      }
      break;
    }
    case 2: {
      const long long* p = (const long long*)plane;
      if (vec) {
        const longlong2 a = *(const longlong2*)(p + i0), c = *(const longlong2*)(p + i0 + 2);
        v[0] = a.x, v[1] = a.y, v[2] = c.x, v[3] = c.y;
      } else {
#pragma unroll
        for (int k = 0; k < PQ_PX; ++k) v[k] = i0 + k < n ? p[i0 + k] : 0;
      }
      break;
    }
    default: {
      const float* p = (const float*)plane;
      if (vec) {
        const float4 q = *(const float4*)(p + i0);
        v[0] = pq_f32(q.x), v[1] = pq_f32(q.y), v[2] = pq_f32(q.z), v[3] = pq_f32(q.w);
      } else {
#pragma unroll
        for (int k = 0; k < PQ_PX; ++k) v[k] = i0 + k < n ? pq_f32(p[i0 + k]) : 0;
      }
      break;
    }
  }
}

__device__ __forceinline__ void pq_load_mask(const float* __restrict__ p, long long i0, long long n, bool vec,
                                             float v[PQ_PX]) {
  if (vec) {
    const float4 q = *(const float4*)(p + i0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < PQ_PX; ++k) v[k] = i0 + k < n ? p[i0 + k] : 1.0f;
  }
}

__device__ __forceinline__ const void* pq_at(const void* p, int kind, size_t elems) {
  const int es = kind == 0 ? 1 : (kind == 2 ? 8 : 4);
  return (const void*)((const char*)p + elems * (size_t)es);
}

__device__ __forceinline__ int wave_or_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// the pixels of one lane and step, decoded: what both walks share
struct PqPixels {
  int pid[PQ_PX], pc[PQ_PX], gid[PQ_PX], gc[PQ_PX];   // -1: outside its domain; gid / gc are -1 on void pixels too
  bool in[PQ_PX], isvoid[PQ_PX];
  int flags;
};

__device__ __forceinline__ void pq_decode(const PqPlanes& pl, size_t plane0, long long i0, long long hw, bool vec,
                                          int n_class, int ignore, PqPixels& px) {
  long long ps[PQ_PX], pc[PQ_PX], gs[PQ_PX], gc[PQ_PX];
  float m[PQ_PX];
  pq_load4(pq_at(pl.pseg, pl.pseg_kind, plane0), pl.pseg_kind, i0, hw, vec, ps);
  pq_load4(pq_at(pl.pcls, pl.pcls_kind, plane0), pl.pcls_kind, i0, hw, vec, pc);
  pq_load4(pq_at(pl.gseg, pl.gseg_kind, plane0), pl.gseg_kind, i0, hw, vec, gs);
  pq_load4(pq_at(pl.gcls, pl.gcls_kind, plane0), pl.gcls_kind, i0, hw, vec, gc);
  if (pl.mask) pq_load_mask(pl.mask + plane0, i0, hw, vec, m);
  px.flags = 0;
#pragma unroll
  for (int k = 0; k < PQ_PX; ++k) {
    px.in[k] = i0 + k < hw;
    px.pid[k] = px.pc[k] = px.gid[k] = px.gc[k] = -1;
    px.isvoid[k] = true;
    if (!px.in[k]) continue;
    if (ps[k] >= 0 && ps[k] < PQ_IDS) px.pid[k] = (int)ps[k];
    else px.flags |= HIM_PQ_ID_RANGE;
    if (pc[k] >= 0 && pc[k] < n_class) px.pc[k] = (int)pc[k];
    else px.flags |= HIM_PQ_CLS_RANGE;
    px.isvoid[k] = (pl.mask && m[k] == 0.0f) || (ignore >= 0 && gc[k] == (long long)ignore);
    if (px.isvoid[k]) continue;
    if (gs[k] >= 0 && gs[k] < PQ_IDS) px.gid[k] = (int)gs[k];
    else px.flags |= HIM_PQ_ID_RANGE;
    if (gc[k] >= 0 && gc[k] < n_class) px.gc[k] = (int)gc[k];
    else px.flags |= HIM_PQ_CLS_RANGE;
  }
}

__global__ __launch_bounds__(256) void pq_clear_kernel(uint4* __restrict__ p, size_t n16) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// the run of a lane that is still open at the end of its share: one add per wave when the wave holds one id
__device__ __forceinline__ void pq_flush_area(unsigned* __restrict__ table, int cur, int cnt) {
  const int first = __builtin_amdgcn_readfirstlane(cur);
  if (__all(cur == first)) {
    const int total = wave_sum_i32(cnt);
    if (first >= 0 && (threadIdx.x & 63) == 0) atomicAdd(&table[first], (unsigned)total);
  } else if (cur >= 0) {
    atomicAdd(&table[cur], (unsigned)cnt);
  }
}

// workgroup (x, b) owns the groups [x * per, (x + 1) * per) of PQ_PX pixels of plane b; per is a multiple of 256
__global__ __launch_bounds__(256) void pq_segment_kernel(PqPlanes pl, long long hw, int vec, int n_class, int ignore,
                                                         long long per, unsigned* __restrict__ hdr,
                                                         unsigned* __restrict__ area) {
  const int tid = threadIdx.x, b = blockIdx.y;
  const size_t plane0 = (size_t)b * (size_t)hw;
  unsigned* ap = area + ((size_t)b * 2 + 1) * PQ_IDS;   // side 1: prediction
  unsigned* ag = area + ((size_t)b * 2 + 0) * PQ_IDS;   // side 0: ground truth
  const long long groups = (hw + PQ_PX - 1) / PQ_PX;
  const long long g0 = blockIdx.x * per, g1 = min(g0 + per, groups);
  int cur_p = -1, cnt_p = 0, cur_g = -1, cnt_g = 0, flags = 0;
  for (long long gb = g0; gb < g1; gb += 256) {
    const long long g = gb + tid;
    if (g >= g1) continue;
    PqPixels px;
    pq_decode(pl, plane0, g * PQ_PX, hw, vec != 0, n_class, ignore, px);
    flags |= px.flags;
#pragma unroll
    for (int k = 0; k < PQ_PX; ++k) {
      if (px.pid[k] >= 0) {
        if (px.pid[k] != cur_p) {
          if (cnt_p) atomicAdd(&ap[cur_p], (unsigned)cnt_p);
          cur_p = px.pid[k], cnt_p = 0;
        }
        ++cnt_p;
      }
      if (px.gid[k] >= 0) {
        if (px.gid[k] != cur_g) {
          if (cnt_g) atomicAdd(&ag[cur_g], (unsigned)cnt_g);
          cur_g = px.gid[k], cnt_g = 0;
        }
        ++cnt_g;
      }
    }
  }
  pq_flush_area(ap, cur_p, cnt_p);
  pq_flush_area(ag, cur_g, cnt_g);
  flags = wave_or_i32(flags);
  if (flags && (tid & 63) == 0) atomicOr(&hdr[4 * b], (unsigned)flags);
}

// workgroup (side, b): dense ranks of the present ids in ascending id
__global__ __launch_bounds__(PQ_RANK_T) void pq_rank_kernel(const unsigned* __restrict__ area, unsigned* __restrict__ rank,
                                                            unsigned* __restrict__ seg, unsigned* __restrict__ hdr, int M,
                                                            int ms) {
  __shared__ int wsum[PQ_RANK_T / 64];
  const int tid = threadIdx.x, side = blockIdx.x, b = blockIdx.y;
  constexpr int PER = PQ_IDS / PQ_RANK_T;
  const size_t t0 = ((size_t)b * 2 + side) * PQ_IDS;
  const uint4* src = (const uint4*)(area + t0 + (size_t)tid * PER);
  unsigned a[PER];
#pragma unroll
  for (int k = 0; k < PER / 4; ++k) {
    const uint4 q = src[k];
    a[4 * k] = q.x, a[4 * k + 1] = q.y, a[4 * k + 2] = q.z, a[4 * k + 3] = q.w;
  }
  int mine = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) mine += a[k] != 0u;
  int incl = mine;   // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += up;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < PQ_RANK_T / 64; ++w) {
    if (w < (tid >> 6)) base += wsum[w];
    total += wsum[w];
  }
  int r = base + incl - mine;
  unsigned* rk = rank + t0 + (size_t)tid * PER;
  unsigned* ids = seg + ((size_t)b * 4 + (size_t)side * 2) * ms;
  unsigned* areas = ids + ms;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (a[k] == 0u) continue;
    rk[k] = (unsigned)r;
    if (r < M) ids[r] = (unsigned)(tid * PER + k), areas[r] = a[k];
    ++r;
  }
  if (tid == 0) {
    hdr[4 * b + 1 + side] = (unsigned)total;
    if (total > M) atomicOr(&hdr[4 * b], (unsigned)HIM_PQ_OVERFLOW);
  }
}

__global__ __launch_bounds__(256) void pq_clear_pair_kernel(const unsigned* __restrict__ hdr, int* __restrict__ pair,
                                                            size_t pair_stride, int* __restrict__ aux, int ms) {
  const int b = blockIdx.y;
  if (hdr[4 * b] & PQ_REFUSED) return;
  const size_t cells = ((size_t)hdr[4 * b + 1] + 1) * (size_t)hdr[4 * b + 2];
  int* p = pair + (size_t)b * pair_stride;
  int* a = aux + (size_t)b * 5 * ms;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) p[i] = 0;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < (size_t)5 * ms; i += (size_t)gridDim.x * 256) a[i] = 0;
}

struct PqRun {
  int key, cnt, grow, prank, gmin, gmax, pmin, pmax;
};

__device__ __forceinline__ void pq_flush_pair(const PqRun& r, int* __restrict__ pair, int* __restrict__ aux, int ms) {
  atomicAdd(&pair[r.key], r.cnt);
  atomicMax(&aux[2 * ms + r.prank], 256 - r.pmin);
  atomicMax(&aux[3 * ms + r.prank], r.pmax + 1);
  if (r.grow > 0) {
    atomicMax(&aux[r.grow - 1], 256 - r.gmin);
    atomicMax(&aux[ms + r.grow - 1], r.gmax + 1);
  }
}

__global__ __launch_bounds__(256) void pq_pair_kernel(PqPlanes pl, long long hw, int vec, int n_class, int ignore,
                                                      long long per, const unsigned* __restrict__ hdr,
                                                      const unsigned* __restrict__ rank, int* __restrict__ pair,
                                                      size_t pair_stride, int* __restrict__ aux, int ms) {
  const int tid = threadIdx.x, b = blockIdx.y;
  if (hdr[4 * b] & PQ_REFUSED) return;   // uniform for the workgroup
  const int ng = (int)hdr[4 * b + 1], np = (int)hdr[4 * b + 2];
  const size_t plane0 = (size_t)b * (size_t)hw;
  const unsigned* rg = rank + ((size_t)b * 2 + 0) * PQ_IDS;
  const unsigned* rp = rank + ((size_t)b * 2 + 1) * PQ_IDS;
  pair += (size_t)b * pair_stride;
  aux += (size_t)b * 5 * ms;
  const long long groups = (hw + PQ_PX - 1) / PQ_PX;
  const long long g0 = blockIdx.x * per, g1 = min(g0 + per, groups);
  PqRun run;
  run.key = -1, run.cnt = 0, run.grow = 0, run.prank = 0, run.gmin = run.pmin = 255, run.gmax = run.pmax = 0;
  int last_pid = -1, last_prank = 0, last_gid = -1, last_grank = 0;
  for (long long gb = g0; gb < g1; gb += 256) {
    const long long g = gb + tid;
    if (g >= g1) continue;
    PqPixels px;
    pq_decode(pl, plane0, g * PQ_PX, hw, vec != 0, n_class, ignore, px);
#pragma unroll
    for (int k = 0; k < PQ_PX; ++k) {
      if (!px.in[k] || px.pid[k] < 0 || px.pc[k] < 0) continue;            // cannot happen on a plane without flags
      if (!px.isvoid[k] && (px.gid[k] < 0 || px.gc[k] < 0)) continue;
      if (px.pid[k] != last_pid) last_pid = px.pid[k], last_prank = (int)rp[last_pid];
      int grow = 0;
      if (!px.isvoid[k]) {
        if (px.gid[k] != last_gid) last_gid = px.gid[k], last_grank = (int)rg[last_gid];
        grow = last_grank + 1;
      }
      if (last_prank >= np || grow > ng) continue;                         // never index past the plane's table
      const int key = grow * np + last_prank;
      if (key != run.key) {
        if (run.cnt) pq_flush_pair(run, pair, aux, ms);
        run.key = key, run.cnt = 0, run.grow = grow, run.prank = last_prank;
        run.gmin = run.pmin = 255, run.gmax = run.pmax = 0;
      }
      ++run.cnt;
      run.pmin = min(run.pmin, px.pc[k]), run.pmax = max(run.pmax, px.pc[k]);
      if (grow > 0) run.gmin = min(run.gmin, px.gc[k]), run.gmax = max(run.gmax, px.gc[k]);
    }
  }
  const int first = __builtin_amdgcn_readfirstlane(run.key);
  if (__all(run.key == first)) {
    if (first < 0) return;
    PqRun all = run;
    all.cnt = wave_sum_i32(run.cnt);
    all.pmin = 255 - wave_max_i32(255 - run.pmin), all.pmax = wave_max_i32(run.pmax);
    all.gmin = 255 - wave_max_i32(255 - run.gmin), all.gmax = wave_max_i32(run.gmax);
    if ((tid & 63) == 0) pq_flush_pair(all, pair, aux, ms);
  } else if (run.cnt) {
    pq_flush_pair(run, pair, aux, ms);
  }
}

// wave (x * 4 + w, b): ground-truth row g of plane b
__global__ __launch_bounds__(256) void pq_match_kernel(const unsigned* __restrict__ hdr, const unsigned* __restrict__ seg,
                                                       const int* __restrict__ pair, size_t pair_stride,
                                                       int* __restrict__ aux, int* __restrict__ res, int M, int ms,
                                                       int* __restrict__ matches) {
  const int lane = threadIdx.x & 63, b = blockIdx.y, g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (hdr[4 * b] & PQ_REFUSED) return;
  const int ng = (int)hdr[4 * b + 1], np = (int)hdr[4 * b + 2];
  if (g >= ng || g >= M) return;
  const unsigned* sg = seg + (size_t)b * 4 * ms;
  const unsigned* sp = sg + 2 * ms;
  pair += (size_t)b * pair_stride;
  aux += (size_t)b * 5 * ms;
  res += (size_t)b * 3 * ms;
  const long long ga = (long long)sg[ms + g];
  const int gc = 256 - aux[g];
  const int* row = pair + (size_t)(g + 1) * np;
  int found = -1, f_inter = 0, f_union = 0;
  for (int p = lane; p < np; p += 64) {
    const long long inter = row[p];
    if (inter <= 0) continue;
    const long long uni = ga + (long long)sp[ms + p] - inter - (long long)pair[p];
    if (256 - aux[2 * ms + p] == gc && 2 * inter > uni && found < 0) found = p, f_inter = (int)inter, f_union = (int)uni;
  }
  const unsigned long long hit = __ballot(found >= 0);
  int m_p = -1, m_inter = 0, m_union = 0;
  if (hit) {
    const int src = __ffsll((long long)hit) - 1;
    m_p = __shfl(found, src, 64), m_inter = __shfl(f_inter, src, 64), m_union = __shfl(f_union, src, 64);
  }
  if (lane == 0) {
    res[g] = m_p, res[ms + g] = m_inter, res[2 * ms + g] = m_union;
    if (m_p >= 0) aux[4 * ms + m_p] = 1;
    if (matches) {
      int* out = matches + ((size_t)b * M + g) * 6;
      out[0] = (int)sg[g], out[1] = gc, out[2] = (int)ga, out[3] = m_p >= 0 ? (int)sp[m_p] : -1, out[4] = m_inter;
      out[5] = m_union;
    }
  }
}

// workgroups [0, cblocks): wave = class.  workgroups cblocks + b: the status row of plane b.
__global__ __launch_bounds__(256) void pq_reduce_kernel(const unsigned* __restrict__ hdr, const unsigned* __restrict__ seg,
                                                        const int* __restrict__ pair, size_t pair_stride,
                                                        const int* __restrict__ aux, const int* __restrict__ res, int B,
                                                        int ms, int n_class, int cblocks, int accumulate,
                                                        long long* __restrict__ counts, double* __restrict__ iou_sum,
                                                        int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  if ((int)blockIdx.x >= cblocks) {
    const int b = blockIdx.x - cblocks;
    int flags = (int)hdr[4 * b];
    const int ng = (int)hdr[4 * b + 1], np = (int)hdr[4 * b + 2];
    int mixed = 0;
    if (!(flags & PQ_REFUSED)) {
      const int* a = aux + (size_t)b * 5 * ms;
      for (int i = threadIdx.x; i < ng; i += 256) mixed |= (256 - a[i]) != (a[ms + i] - 1);
      for (int i = threadIdx.x; i < np; i += 256) mixed |= (256 - a[2 * ms + i]) != (a[3 * ms + i] - 1);
    }
    if (__syncthreads_or(mixed)) flags |= HIM_PQ_MIXED;
    if (threadIdx.x == 0) {
      int* s = status + 4 * b;
      if (accumulate) s[0] += ng, s[1] += np, s[2] |= flags;
      else s[0] = ng, s[1] = np, s[2] = flags, s[3] = 0;
    }
    return;
  }
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_class) return;
  int tp = 0, fp = 0, fn = 0;
  double iou = 0.0;
  for (int b = 0; b < B; ++b) {
    if (hdr[4 * b] & PQ_REFUSED) continue;
    const int ng = (int)hdr[4 * b + 1], np = (int)hdr[4 * b + 2];
    const unsigned* sp = seg + (size_t)b * 4 * ms + 2 * ms;
    const int* a = aux + (size_t)b * 5 * ms;
    const int* r = res + (size_t)b * 3 * ms;
    const int* voidrow = pair + (size_t)b * pair_stride;
    for (int g = lane; g < ng; g += 64) {
      if (256 - a[g] != c) continue;
      if (r[g] >= 0) ++tp, iou += (double)r[ms + g] / (double)r[2 * ms + g];
      else ++fn;
    }
    for (int p = lane; p < np; p += 64) {
      if (256 - a[2 * ms + p] != c || a[4 * ms + p]) continue;
      if (2LL * (long long)voidrow[p] > (long long)sp[ms + p]) continue;
      ++fp;
    }
  }
  tp = wave_sum_i32(tp), fp = wave_sum_i32(fp), fn = wave_sum_i32(fn);
  iou = wave_sum_f64(iou);
  if (lane == 0) {
    if (accumulate) {
      counts[3 * c] += tp, counts[3 * c + 1] += fp, counts[3 * c + 2] += fn;
      iou_sum[c] += iou;
    } else {
      counts[3 * c] = tp, counts[3 * c + 1] = fp, counts[3 * c + 2] = fn;
      iou_sum[c] = iou;
    }
  }
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

size_t him_panoptic_match_workspace(int B, int max_segments) {
  if (B < 1 || B > 65535 || max_segments < 1 || max_segments > 4096) return 0;
  return pq_layout(B, max_segments).total;
}

int him_panoptic_match(const void* pred_seg, int pred_seg_kind, const void* pred_cls, int pred_cls_kind,
                       const void* gt_seg, int gt_seg_kind, const void* gt_cls, int gt_cls_kind, const float* mask, int B,
                       int H, int W, int n_class, int ignore, int max_segments, int accumulate, long long* counts,
                       double* iou_sum, int* matches, int* status, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL)
    return fail(HIM_E_INVALID, "panoptic_match: bad shape");
  if (n_class < 1 || n_class > 256) return fail(HIM_E_INVALID, "panoptic_match: n_class %d (1..256)", n_class);
  if (max_segments < 1 || max_segments > 4096)
    return fail(HIM_E_INVALID, "panoptic_match: max_segments %d (1..4096)", max_segments);
  if (pred_seg_kind < 0 || pred_seg_kind > 2 || gt_seg_kind < 0 || gt_seg_kind > 2)
    return fail(HIM_E_INVALID, "panoptic_match: segment kinds %d, %d (0..2)", pred_seg_kind, gt_seg_kind);
  if (pred_cls_kind < 0 || pred_cls_kind > 3 || gt_cls_kind < 0 || gt_cls_kind > 3)
    return fail(HIM_E_INVALID, "panoptic_match: class kinds %d, %d (0..3)", pred_cls_kind, gt_cls_kind);
  if (ignore < -1) return fail(HIM_E_INVALID, "panoptic_match: ignore %d (-1 or a class)", ignore);
  if (!pred_seg || !pred_cls || !gt_seg || !gt_cls || !counts || !iou_sum || !status || !ws)
    return fail(HIM_E_INVALID, "panoptic_match: null pointer");
  if ((uintptr_t)ws % 16 != 0) return fail(HIM_E_INVALID, "panoptic_match: workspace not 16-byte aligned");
  if ((uintptr_t)counts % 8 != 0 || (uintptr_t)iou_sum % 8 != 0 || (uintptr_t)status % 4 != 0 || (uintptr_t)matches % 4 != 0)
    return fail(HIM_E_INVALID, "panoptic_match: counts / iou_sum / matches / status misaligned");
  static const int esize[4] = {1, 4, 8, 4};
  if ((uintptr_t)pred_seg % esize[pred_seg_kind] != 0 || (uintptr_t)pred_cls % esize[pred_cls_kind] != 0 ||
      (uintptr_t)gt_seg % esize[gt_seg_kind] != 0 || (uintptr_t)gt_cls % esize[gt_cls_kind] != 0 || (uintptr_t)mask % 4 != 0)
    return fail(HIM_E_INVALID, "panoptic_match: plane not aligned to its element size");
  const PqLayout l = pq_layout(B, max_segments);
  if (ws_bytes < l.total) return fail(HIM_E_WORKSPACE, "panoptic_match: workspace %zu < %zu bytes", ws_bytes, l.total);

  const long long hw = (long long)H * W;
  const int vec = (W % PQ_PX == 0 && (uintptr_t)pred_seg % 16 == 0 && (uintptr_t)pred_cls % 16 == 0 &&
                   (uintptr_t)gt_seg % 16 == 0 && (uintptr_t)gt_cls % 16 == 0 && (uintptr_t)mask % 16 == 0) ? 1 : 0;
  PqPlanes pl;
  pl.pseg = pred_seg, pl.pcls = pred_cls, pl.gseg = gt_seg, pl.gcls = gt_cls, pl.mask = mask;
  pl.pseg_kind = pred_seg_kind, pl.pcls_kind = pred_cls_kind, pl.gseg_kind = gt_seg_kind, pl.gcls_kind = gt_cls_kind;
  char* base = (char*)ws;
  unsigned* hdr = (unsigned*)(base + l.hdr);
  unsigned* area = (unsigned*)(base + l.area);
  unsigned* rank = (unsigned*)(base + l.rank);
  unsigned* seg = (unsigned*)(base + l.seg);
  int* aux = (int*)(base + l.aux);
  int* res = (int*)(base + l.res);
  int* pair = (int*)(base + l.pair);
  const int M = max_segments, ms = (int)l.ms;

  // the walk's shares: at least 512 groups (2 048 pixels) per workgroup, at most 4 workgroups per compute unit in all
  const long long groups = (hw + PQ_PX - 1) / PQ_PX;
  const long long cap = 4LL * device_cus();
  long long wgs = (groups + 511) / 512;
  const long long per_b = cap / B > 0 ? cap / B : 1;
  if (wgs > per_b) wgs = per_b;
  if (wgs < 1) wgs = 1;
  long long per = (groups + wgs - 1) / wgs;
  per = (per + 255) / 256 * 256;
  wgs = (groups + per - 1) / per;
  const dim3 walk((unsigned)wgs, (unsigned)B);

  const size_t n16 = (l.rank - l.hdr) / 16;   // header and area tables are adjacent
  hipLaunchKernelGGL(pq_clear_kernel, dim3((unsigned)(n16 / 256 > 1024 ? 1024 : (n16 + 255) / 256)), dim3(256), 0, ST,
                     (uint4*)(base + l.hdr), n16);
  hipLaunchKernelGGL(pq_segment_kernel, walk, dim3(256), 0, ST, pl, hw, vec, n_class, ignore, per, hdr, area);
  hipLaunchKernelGGL(pq_rank_kernel, dim3(2, B), dim3(PQ_RANK_T), 0, ST, (const unsigned*)area, rank, seg, hdr, M, ms);
  const size_t cells = ((size_t)M + 1) * M;
  hipLaunchKernelGGL(pq_clear_pair_kernel, dim3((unsigned)(cells / 4096 > 128 ? 128 : cells / 4096 + 1), B), dim3(256), 0,
                     ST, (const unsigned*)hdr, pair, l.pair_stride, aux, ms);
  hipLaunchKernelGGL(pq_pair_kernel, walk, dim3(256), 0, ST, pl, hw, vec, n_class, ignore, per, (const unsigned*)hdr,
                     (const unsigned*)rank, pair, l.pair_stride, aux, ms);
  hipLaunchKernelGGL(pq_match_kernel, dim3((M + 3) / 4, B), dim3(256), 0, ST, (const unsigned*)hdr, (const unsigned*)seg,
                     (const int*)pair, l.pair_stride, aux, res, M, ms, matches);
  const int cblocks = (n_class + 3) / 4;
  hipLaunchKernelGGL(pq_reduce_kernel, dim3(cblocks + B), dim3(256), 0, ST, (const unsigned*)hdr, (const unsigned*)seg,
                     (const int*)pair, l.pair_stride, (const int*)aux, (const int*)res, B, ms, n_class, cblocks,
                     accumulate ? 1 : 0, counts, iou_sum, status);
  return check_launch("panoptic_match");
}

}  // extern "C"
