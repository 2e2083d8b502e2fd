// Loader-side pixel work on the device: crop windows of label / instance maps and photographs arrive as raw bytes,
// everything the reference's loader does to them afterwards (data/base_dataset.py:243-268 -> PIL.Image.resize,
// FLIP_LEFT_RIGHT, ToTensor, Normalize; data/segmentation_dataset.py:86-131 masks) happens here in four launches per
// batch.  Byte / integer work, HBM-bound and tiny next to the training step; the point is that the batch is born on
// the device in the trainer's compact layout and that the bytes equal Pillow's (the index / weight tables come from
// data/resample.py, the arithmetic below is Pillow's 8-bit fixed point: Resample.c ImagingResampleHorizontal_8bpc).
#include "him_common.h"

namespace him {

#define DATA_PRECISION_BITS 22

__device__ __forceinline__ int clip8(int v) {
  v >>= DATA_PRECISION_BITS;  // arithmetic shift, as Pillow's clip8_lookups index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// out[b][y][x] = src_b[ytab[b][y]][xtab[b][x]]   (a flip is already folded into xtab)
template <typename SRC>
__global__ void data_nearest_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ off,
                                    const int* __restrict__ pitch, const int* __restrict__ xtab,
                                    const int* __restrict__ ytab, void* __restrict__ dst, int dst_kind, int B, int H,
                                    int W) {
  long long n = (long long)B * H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    int x = (int)(i % W);
    long long r = i / W;
    int y = (int)(r % H);
    int b = (int)(r / H);
    const SRC* s = (const SRC*)(base + off[b]);
    SRC v = s[(long long)ytab[b * H + y] * pitch[b] + xtab[b * W + x]];
    switch (dst_kind) {
      case 0: ((float*)dst)[i] = (float)v; break;                       // ToTensor()*255 of an 8-bit map is the id itself
      case 1: ((float*)dst)[i] = __fdiv_rn((float)v, 255.f); break;     // ToTensor() of an 8-bit map
      case 2: ((unsigned char*)dst)[i] = (unsigned char)v; break;       // compact ids for the trainer's uint8 input
      default: ((int*)dst)[i] = (int)v; break;                          // ToTensor() of an integer-mode map
    }
  }
}

// The same gather from a map kept as per-row run lists (preprocess_pack.py): image b has row_start[h+1] (runs of row r
// are [row_start[r], row_start[r+1])), run_x[n] (first column of a run, 0 for the first run of a row, ascending inside
// a row) and run_v[n] (its value), each at a byte offset from `base`.  out[b][y][x] = value of the last run of row
// y0[b] + ytab[b][y] whose start is <= x0[b] + xtab[b][x].  A lane owns RLE_PX adjacent outputs of one row: it searches
// the row's runs for the first, and keeps the run it found for the next ones while their column stays inside it (xtab
// is monotone, so neighbours mostly share a run); otherwise it searches again.  The search never leaves the row's
// [row_start[r], row_start[r+1]); an empty range gives 0.  `vec` (host: W % RLE_PX == 0 and dst aligned to RLE_PX
// elements): the lane's outputs leave in one store; otherwise element stores, bounds-checked.
#define RLE_PX 4

template <typename T>
__device__ __forceinline__ void rle_store(void* __restrict__ dst, long long i0, int m, bool vec, const T v[RLE_PX]) {
  if (vec) {
    struct alignas(RLE_PX * sizeof(T)) Q { T a[RLE_PX]; };
    Q q;
#pragma unroll
    for (int k = 0; k < RLE_PX; ++k) q.a[k] = v[k];
    *(Q*)((T*)dst + i0) = q;
  } else {
#pragma unroll
    for (int k = 0; k < RLE_PX; ++k)
      if (k < m) ((T*)dst)[i0 + k] = v[k];
  }
}

__global__ void data_nearest_rle_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ row_off,
                                        const long long* __restrict__ runx_off, const long long* __restrict__ runv_off,
                                        const int* __restrict__ x0, const int* __restrict__ y0,
                                        const int* __restrict__ xtab, const int* __restrict__ ytab,
                                        void* __restrict__ dst, int dst_kind, int vec, int B, int H, int W) {
  const int gw = (W + RLE_PX - 1) / RLE_PX;  // groups per output row
  const long long groups = (long long)B * H * gw;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const int xg = (int)(g % gw) * RLE_PX;
    const long long r = g / gw;
    const int y = (int)(r % H);
    const int b = (int)(r / H);
    const int m = W - xg < RLE_PX ? W - xg : RLE_PX;  // outputs of this group inside the row
    const int* rs = (const int*)(base + row_off[b]);
    const int* rx = (const int*)(base + runx_off[b]);
    const int* rv = (const int*)(base + runv_off[b]);
    const int row = y0[b] + ytab[b * H + y];
    const int lo = rs[row], hi = rs[row + 1];
    int xs = 1, xe = 0, val = 0;  // the run in hand covers columns [xs, xe): none yet
    int v[RLE_PX];
#pragma unroll
    for (int k = 0; k < RLE_PX; ++k) {
      v[k] = 0;
      if (k < m) {
        const int col = x0[b] + xtab[b * W + xg + k];
        if ((col < xs || col >= xe) && hi > lo) {
          int a = lo, n = hi - lo;  // the answer lies in [a, a + n)
          while (n > 1) {
            const int h = n >> 1;
            if (rx[a + h] <= col) { a += h; n -= h; } else n = h;
          }
          xs = rx[a];
          xe = a + 1 < hi ? rx[a + 1] : 0x7fffffff;
          val = rv[a];
        }
        v[k] = val;
      }
    }
    const long long i0 = ((long long)b * H + y) * W + xg;
    switch (dst_kind) {  // the conversions of data_nearest_kernel
      case 0: {
        float f[RLE_PX];
#pragma unroll
        for (int k = 0; k < RLE_PX; ++k) f[k] = (float)v[k];
        rle_store(dst, i0, m, vec != 0, f);
        break;
      }
      case 1: {
        float f[RLE_PX];
#pragma unroll
        for (int k = 0; k < RLE_PX; ++k) f[k] = __fdiv_rn((float)v[k], 255.f);
        rle_store(dst, i0, m, vec != 0, f);
        break;
      }
      case 2: {
        unsigned char c[RLE_PX];
#pragma unroll
        for (int k = 0; k < RLE_PX; ++k) c[k] = (unsigned char)v[k];
        rle_store(dst, i0, m, vec != 0, c);
        break;
      }
      default: rle_store(dst, i0, m, vec != 0, v); break;
    }
  }
}

// horizontal pass over interleaved RGB bytes: tmp[b][r][i][c] = clip8(2^21 + sum_k w[b][i][k] * src_b[r][first+k][c])
__global__ void data_bicubic_h_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ off,
                                      const int* __restrict__ pitch, const int* __restrict__ rows,
                                      const int* __restrict__ first, const int* __restrict__ count,
                                      const int* __restrict__ weights, int ksize, unsigned char* __restrict__ tmp,
                                      int maxrows, int B, int W) {
  int b = blockIdx.z;
  int r = blockIdx.y;
  if (r >= rows[b]) return;
  const unsigned char* s = base + off[b] + (long long)r * pitch[b] * 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += gridDim.x * blockDim.x) {
    int f = first[b * W + i], n = count[b * W + i];
    const int* w = weights + ((long long)b * W + i) * ksize;
    int a0 = 1 << (DATA_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < n; ++k) {
      int wk = w[k];
      const unsigned char* p = s + (f + k) * 3;
      a0 += (int)p[0] * wk;
      a1 += (int)p[1] * wk;
      a2 += (int)p[2] * wk;
    }
    unsigned char* o = tmp + (((long long)b * maxrows + r) * W + i) * 3;
    o[0] = (unsigned char)clip8(a0);
    o[1] = (unsigned char)clip8(a1);
    o[2] = (unsigned char)clip8(a2);
  }
}

// vertical pass + FLIP_LEFT_RIGHT + ToTensor + Normalize(.5,.5): dst[b][c][y][x'] = ((v / 255) - .5) / .5
__global__ void data_bicubic_v_kernel(const unsigned char* __restrict__ tmp, int maxrows,
                                      const int* __restrict__ first, const int* __restrict__ count,
                                      const int* __restrict__ weights, int ksize, const int* __restrict__ flip,
                                      float* __restrict__ dst, int normalize, int B, int H, int W) {
  int b = blockIdx.z;
  int y = blockIdx.y;
  int f = first[b * H + y], n = count[b * H + y];
  const int* w = weights + ((long long)b * H + y) * ksize;
  for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < W; x += gridDim.x * blockDim.x) {
    int a0 = 1 << (DATA_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < n; ++k) {
      int wk = w[k];
      const unsigned char* p = tmp + (((long long)b * maxrows + f + k) * W + x) * 3;
      a0 += (int)p[0] * wk;
      a1 += (int)p[1] * wk;
      a2 += (int)p[2] * wk;
    }
    int xo = flip[b] ? W - 1 - x : x;
    int v[3] = {clip8(a0), clip8(a1), clip8(a2)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t = __fdiv_rn((float)v[c], 255.f);
      if (normalize) t = __fdiv_rn(__fsub_rn(t, 0.5f), 0.5f);
      dst[(((long long)b * 3 + c) * H + y) * W + xo] = t;
    }
  }
}

// get_masked_image for the input and the output window + the instance mask, one pass (segmentation_dataset.py:95-131)
__global__ void data_region_masks_kernel(const float* __restrict__ label, const void* __restrict__ inst, int inst_kind,
                                         const int* __restrict__ boxes, const float* __restrict__ fill,
                                         const int* __restrict__ inst_id, float* __restrict__ mask_in,
                                         float* __restrict__ obj_in, float* __restrict__ ctx_in,
                                         float* __restrict__ mask_out, float* __restrict__ obj_out,
                                         float* __restrict__ inst_mask, int B, int H, int W) {
  long long n = (long long)B * H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    int x = (int)(i % W);
    long long r = i / W;
    int y = (int)(r % H);
    int b = (int)(r / H);
    const int* q = boxes + b * 8;  // (wmin, hmin, wmax, hmax) of the input window, then of the output window
    float mi = (q[3] > q[1] && q[2] > q[0] && y >= q[1] && y < q[3] && x >= q[0] && x < q[2]) ? 1.f : 0.f;
    float mo = (q[7] > q[5] && q[6] > q[4] && y >= q[5] && y < q[7] && x >= q[4] && x < q[6]) ? 1.f : 0.f;
    float l = label[i];
    mask_in[i] = mi;
    obj_in[i] = mi * l;
    ctx_in[i] = (1.f - mi) * l + mi * fill[b];
    mask_out[i] = mo;
    obj_out[i] = mo * l;
    if (inst_mask) {
      float m = 0.f;
      if (inst_id[b * 2]) {  // [b][0] = "an instance was selected", [b][1] = its id
        if (inst_kind == 0) m = ((const float*)inst)[i] == (float)inst_id[b * 2 + 1] ? 1.f : 0.f;
        else m = ((const int*)inst)[i] == inst_id[b * 2 + 1] ? 1.f : 0.f;
      }
      inst_mask[i] = m;
    }
  }
}

// ---- canvas crop / paste of the joint inference (util/data_util.py crop_canvas / paste_canvas upstream) ----------
// ToPILImage of a window of C fp32 planes (Hs, Ws): byte = trunc(pre(v) * 255) with pre 0: v, 1: v / 255 (a label map
// through tensor2pil), 2: (v + 1) / 2 (the generator's tanh output); each operation rounded on its own, no contraction.
// Pixels of the window outside the planes are 0 (Image.crop's fill).  dst (h, w, C) interleaved bytes.
__global__ void canvas_window_bytes_kernel(const float* __restrict__ src, int C, int Hs, int Ws, int x0, int y0, int h,
                                           int w, int pre, unsigned char* __restrict__ dst) {
  long long n = (long long)h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int sx = x0 + (int)(i % w), sy = y0 + (int)(i / w);
    const bool inside = sx >= 0 && sx < Ws && sy >= 0 && sy < Hs;
    for (int c = 0; c < C; ++c) {
      unsigned char b = 0;
      if (inside) {
        float v = src[((long long)c * Hs + sy) * Ws + sx];
        if (pre == 1) v = __fdiv_rn(v, 255.f);
        else if (pre == 2) v = __fdiv_rn(__fadd_rn(v, 1.f), 2.f);
        b = (unsigned char)(int)__fmul_rn(v, 255.f);   // Tensor.byte(): truncation
      }
      dst[i * C + c] = b;
    }
  }
}

// vertical BICUBIC pass of a (rows, W, 3) byte image written as ToTensor (v / 255) into a window of a (3, Hc, Wc) canvas
__global__ void canvas_paste_bicubic_v_kernel(const unsigned char* __restrict__ tmp, const int* __restrict__ first,
                                              const int* __restrict__ count, const int* __restrict__ weights, int ksize,
                                              float* __restrict__ canvas, int Hc, int Wc, int x0, int y0, int W) {
  const int y = blockIdx.y;
  const int f = first[y], n = count[y];
  const int* w = weights + (long long)y * ksize;
  for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < W; x += gridDim.x * blockDim.x) {
    int a0 = 1 << (DATA_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < n; ++k) {
      const int wk = w[k];
      const unsigned char* p = tmp + ((long long)(f + k) * W + x) * 3;
      a0 += (int)p[0] * wk;
      a1 += (int)p[1] * wk;
      a2 += (int)p[2] * wk;
    }
    const int v[3] = {clip8(a0), clip8(a1), clip8(a2)};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      canvas[((long long)c * Hc + y0 + y) * Wc + x0 + x] = __fdiv_rn((float)v[c], 255.f);
  }
}

// window copy of C planes (h, w) (f32 or i64, converted to f32) into a (C, Hc, Wc) canvas at (x0, y0)
__global__ void canvas_paste_window_kernel(const void* __restrict__ src, int src_kind, int C, int h, int w,
                                           float* __restrict__ canvas, int Hc, int Wc, int x0, int y0) {
  long long n = (long long)C * h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    const long long r = i / w;
    const int y = (int)(r % h), c = (int)(r / h);
    const float v = src_kind ? (float)((const long long*)src)[i] : ((const float*)src)[i];
    canvas[((long long)c * Hc + y0 + y) * Wc + x0 + x] = v;
  }
}

static inline dim3 data_grid(long long n) {
  long long g = (n + 255) / 256;
  return dim3((unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g)));
}

// ---- tensors to pictures (util/util.py tensor2im / tensor2label / tensor2seglabel upstream) ------------------------
// One pass each, HBM-bound.  A thread owns VIS_PX adjacent pixels of the flattened (H*W) plane: one 16-byte load per
// channel plane, and the interleaved bytes of its pixels leave as whole dwords (4 RGB pixels = 3 dwords).  `vec` (host:
// H*W % 4 == 0 and a 16-byte aligned base, so every plane is aligned and every group full) selects the wide loads,
// `packed` (host: dst 4-byte aligned) the dword stores; otherwise element loads / byte stores, bounds-checked.
#define VIS_PX 4

template <typename T>
__device__ __forceinline__ void vis_load4(const T* __restrict__ plane, long long i0, long long n, bool vec, T v[VIS_PX]) {
  if (vec) {
    struct alignas(VIS_PX * sizeof(T)) Q { T a[VIS_PX]; };
    const Q q = *(const Q*)(plane + i0);
#pragma unroll
    for (int k = 0; k < VIS_PX; ++k) v[k] = q.a[k];
  } else {
#pragma unroll
    for (int k = 0; k < VIS_PX; ++k) v[k] = i0 + k < n ? plane[i0 + k] : T(0);
  }
}

// px[k] = r | g << 8 | b << 16 of pixel i0 + k  ->  dst (n, 3) bytes
__device__ __forceinline__ void vis_store_rgb4(unsigned char* __restrict__ dst, long long i0, long long n, bool packed,
                                               const unsigned px[VIS_PX]) {
  if (packed && i0 + VIS_PX <= n) {
    struct alignas(4) W3 { unsigned a, b, c; };
    W3 w;
    w.a = px[0] | (px[1] << 24);
    w.b = (px[1] >> 8) | (px[2] << 16);
    w.c = (px[2] >> 16) | (px[3] << 8);
    *(W3*)(dst + i0 * 3) = w;
  } else {
#pragma unroll
    for (int k = 0; k < VIS_PX; ++k)
      if (i0 + k < n) {
        unsigned char* o = dst + (i0 + k) * 3;
        o[0] = (unsigned char)(px[k] & 255u);
        o[1] = (unsigned char)((px[k] >> 8) & 255u);
        o[2] = (unsigned char)(px[k] >> 16);
      }
  }
}

// tensor2im: byte = trunc(clip(normalize ? (x + 1) / 2 * 255 : x * 255, 0, 255)), every operation rounded to fp32 on
// its own as numpy does (no contraction: the single-FMA form differs in about one value of 1 800)
__device__ __forceinline__ unsigned im_byte(float x, bool normalize) {
  float v = normalize ? __fmul_rn(__fmul_rn(__fadd_rn(x, 1.0f), 0.5f), 255.0f) : __fmul_rn(x, 255.0f);
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (unsigned)(int)v;
}

__global__ void tensor2im_bytes_kernel(const float* __restrict__ src, int C, long long n, int normalize, int vec,
                                       int packed, unsigned char* __restrict__ dst) {
  const long long groups = (n + VIS_PX - 1) / VIS_PX;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i0 = g * VIS_PX;
    float r[VIS_PX];
    unsigned px[VIS_PX];
    vis_load4(src, i0, n, vec != 0, r);
    if (C == 1) {  // upstream repeats a 1-channel tensor to 3 channels
#pragma unroll
      for (int k = 0; k < VIS_PX; ++k) px[k] = im_byte(r[k], normalize != 0) * 0x010101u;
    } else {
      float gch[VIS_PX], b[VIS_PX];
      vis_load4(src + n, i0, n, vec != 0, gch);
      vis_load4(src + 2 * n, i0, n, vec != 0, b);
#pragma unroll
      for (int k = 0; k < VIS_PX; ++k)
        px[k] = im_byte(r[k], normalize != 0) | (im_byte(gch[k], normalize != 0) << 8) | (im_byte(b[k], normalize != 0) << 16);
    }
    vis_store_rgb4(dst, i0, n, packed != 0, px);
  }
}

// Colorize's "label == map" on a float map paints integer values in [0, n) only; everything else stays (0, 0, 0)
__device__ __forceinline__ int vis_label(float v, int n) { return (v >= 0.0f && v < (float)n && v == floorf(v)) ? (int)v : -1; }
__device__ __forceinline__ int vis_label(unsigned char v, int n) { return (int)v < n ? (int)v : -1; }
__device__ __forceinline__ int vis_label(long long v, int n) { return (v >= 0 && v < (long long)n) ? (int)v : -1; }

// tensor2label's label branch: C > 1 (T = float): label = channel of the maximum, the LOWEST channel on a tie (strict >
// walking upwards, what max(0)[1] returns on the host); C == 1: the plane holds the ids.  dst = table[label].
template <typename T>
__global__ void label2color_bytes_kernel(const T* __restrict__ src, int C, long long n, const unsigned char* __restrict__ table,
                                         int ntab, int vec, int packed, unsigned char* __restrict__ dst) {
  extern __shared__ unsigned vis_tab[];  // ntab entries r | g << 8 | b << 16
  for (int i = threadIdx.x; i < ntab; i += blockDim.x)
    vis_tab[i] = (unsigned)table[3 * i] | ((unsigned)table[3 * i + 1] << 8) | ((unsigned)table[3 * i + 2] << 16);
  __syncthreads();
  const long long groups = (n + VIS_PX - 1) / VIS_PX;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i0 = g * VIS_PX;
    int lab[VIS_PX];
    T v[VIS_PX];
    vis_load4(src, i0, n, vec != 0, v);
    if (C == 1) {
#pragma unroll
      for (int k = 0; k < VIS_PX; ++k) lab[k] = vis_label(v[k], ntab);
    } else {
      T best[VIS_PX];
#pragma unroll
      for (int k = 0; k < VIS_PX; ++k) { best[k] = v[k]; lab[k] = 0; }
#pragma unroll 4
      for (int c = 1; c < C; ++c) {
        vis_load4(src + (long long)c * n, i0, n, vec != 0, v);
#pragma unroll
        for (int k = 0; k < VIS_PX; ++k)
          if (v[k] > best[k]) { best[k] = v[k]; lab[k] = c; }
      }
#pragma unroll
      for (int k = 0; k < VIS_PX; ++k) lab[k] = lab[k] < ntab ? lab[k] : -1;
    }
    unsigned px[VIS_PX];
#pragma unroll
    for (int k = 0; k < VIS_PX; ++k) px[k] = lab[k] >= 0 ? vis_tab[lab[k]] : 0u;
    vis_store_rgb4(dst, i0, n, packed != 0, px);
  }
}

// tensor2seglabel: dst[p][c] = trunc(src[c][p]).  CT = 1..4: the CT * VIS_PX bytes of a thread's pixels leave as CT
// dwords; CT = 0: any C, byte stores.
template <int CT>
__global__ void seglabel_bytes_kernel(const float* __restrict__ src, int C, long long n, int vec, int packed,
                                      unsigned char* __restrict__ dst) {
  const long long groups = (n + VIS_PX - 1) / VIS_PX;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i0 = g * VIS_PX;
    float v[VIS_PX];
    if constexpr (CT > 0) {
      unsigned w[CT > 0 ? CT : 1] = {};
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        vis_load4(src + (long long)c * n, i0, n, vec != 0, v);
#pragma unroll
        for (int k = 0; k < VIS_PX; ++k) {
          const int at = k * CT + c;  // byte index inside the thread's CT * VIS_PX output bytes
          w[at >> 2] |= ((unsigned)(int)v[k] & 255u) << ((at & 3) * 8);
        }
      }
      if (packed && i0 + VIS_PX <= n) {
#pragma unroll
        for (int j = 0; j < CT; ++j) ((unsigned*)(dst + i0 * CT))[j] = w[j];
      } else {
#pragma unroll
        for (int at = 0; at < CT * VIS_PX; ++at)
          if (i0 + at / CT < n) dst[i0 * CT + at] = (unsigned char)(w[at >> 2] >> ((at & 3) * 8));
      }
    } else {
      for (int c = 0; c < C; ++c) {
        vis_load4(src + (long long)c * n, i0, n, vec != 0, v);
#pragma unroll
        for (int k = 0; k < VIS_PX; ++k)
          if (i0 + k < n) dst[(i0 + k) * C + c] = (unsigned char)(int)v[k];
      }
    }
  }
}

static inline bool vis_vec(const void* src, long long n, size_t elem) {
  return n % VIS_PX == 0 && (uintptr_t)src % (VIS_PX * elem) == 0;
}
static inline bool vis_packed(const void* dst) { return (uintptr_t)dst % 4 == 0; }
static inline dim3 vis_grid(long long n) { return data_grid((n + VIS_PX - 1) / VIS_PX); }

// ---- instance-box summary (preprocess_city.py construct_box upstream) ---------------------------------------------
// Workspace (ints): box[5][65536] = xmin | ymin | xmax | ymax | count per id, rowmap[65536] = id -> table row or -1,
// hist[max_objects][256] = class counts per table row.  Five launches: clear, box pass, compaction (one workgroup),
// class pass, median.  A lane owns INST_PX adjacent pixels of the flattened plane and folds equal neighbours into runs;
// a workgroup collects its runs in an LDS hash table and touches the global tables once per distinct key (Guideline 12:
// partial reduction first); a key the LDS table has no room for goes to the global table directly.  Integer min / max /
// add only, so arrival order never shows in the result.
#define INST_IDS 65536
#define INST_PX 8
#define INST_BOX_SLOTS 512
#define INST_CLS_SLOTS 1024
#define INST_PROBES 8

__device__ __forceinline__ int inst_id(unsigned char v) { return (int)v; }
__device__ __forceinline__ int inst_id(unsigned short v) { return (int)v; }
__device__ __forceinline__ int inst_id(int v) { return (v >= 0 && v < INST_IDS) ? v : -2; }
__device__ __forceinline__ int inst_id(long long v) { return (v >= 0 && v < INST_IDS) ? (int)v : -2; }
__device__ __forceinline__ int inst_cls(unsigned char v) { return (int)v; }
__device__ __forceinline__ int inst_cls(int v) { return (v >= 0 && v < 256) ? v : -2; }
__device__ __forceinline__ int inst_cls(long long v) { return (v >= 0 && v < 256) ? (int)v : -2; }
__device__ __forceinline__ int inst_cls(float v) { return (v >= 0.0f && v < 256.0f && v == floorf(v)) ? (int)v : -2; }

// v[k] = id / class of pixel i0 + k (-2: outside the accepted domain, -3: behind the plane's end)
template <typename T, typename F>
__device__ __forceinline__ void inst_load(const T* __restrict__ plane, long long i0, long long n, bool vec, F conv,
                                          int v[INST_PX]) {
  if (vec) {
    struct alignas(sizeof(T) * INST_PX < 16 ? sizeof(T) * INST_PX : 16) Q { T a[INST_PX]; };
    const Q q = *(const Q*)(plane + i0);
#pragma unroll
    for (int k = 0; k < INST_PX; ++k) v[k] = conv(q.a[k]);
  } else {
#pragma unroll
    for (int k = 0; k < INST_PX; ++k) v[k] = i0 + k < n ? conv(plane[i0 + k]) : -3;
  }
}

__device__ __forceinline__ int inst_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int inst_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// slot of `key` (>= 0) in an LDS table of SLOTS keys (-1 = free), linear probing; -1: no room within INST_PROBES
template <int SLOTS>
__device__ __forceinline__ int inst_slot(int* keys, int key) {
  const unsigned h = ((unsigned)key * 2654435761u) >> 12;
#pragma unroll 1
  for (int p = 0; p < INST_PROBES; ++p) {
    const int s = (int)((h + p) & (SLOTS - 1));
    const int old = atomicCAS(&keys[s], -1, key);
    if (old == -1 || old == key) return s;
  }
  return -1;
}

__global__ void inst_clear_kernel(int* __restrict__ ws, int nhist, int* __restrict__ status) {
  const int total = 5 * INST_IDS + nhist;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < 2 * INST_IDS) ws[i] = 0x7fffffff;                 // xmin, ymin
    else if (i < 4 * INST_IDS) ws[i] = -1;                    // xmax, ymax
    else if (i < 5 * INST_IDS) ws[i] = 0;                     // count
    else ws[6 * INST_IDS + (i - 5 * INST_IDS)] = 0;           // hist (rowmap is written whole by the compaction)
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) status[threadIdx.x] = 0;
}

struct InstBoxLds {
  int key[INST_BOX_SLOTS], xmin[INST_BOX_SLOTS], ymin[INST_BOX_SLOTS], xmax[INST_BOX_SLOTS], ymax[INST_BOX_SLOTS],
      cnt[INST_BOX_SLOTS];
};

__device__ __forceinline__ void inst_box_add(InstBoxLds& L, int* __restrict__ box, int id, int x0, int x1, int y0,
                                             int y1, int n) {
  const int s = inst_slot<INST_BOX_SLOTS>(L.key, id);
  if (s >= 0) {
    atomicMin(&L.xmin[s], x0);
    atomicMin(&L.ymin[s], y0);
    atomicMax(&L.xmax[s], x1);
    atomicMax(&L.ymax[s], y1);
    atomicAdd(&L.cnt[s], n);
  } else {
    atomicMin(&box[id], x0);
    atomicMin(&box[INST_IDS + id], y0);
    atomicMax(&box[2 * INST_IDS + id], x1);
    atomicMax(&box[3 * INST_IDS + id], y1);
    atomicAdd(&box[4 * INST_IDS + id], n);
  }
}

// workgroup b owns the groups [b * per, (b + 1) * per) of INST_PX pixels
template <typename T>
__global__ __launch_bounds__(256) void inst_box_kernel(const T* __restrict__ inst, int H, int W, int vec, int min_id,
                                                       long long per, int* __restrict__ box, int* __restrict__ status) {
  __shared__ InstBoxLds L;
  for (int s = threadIdx.x; s < INST_BOX_SLOTS; s += blockDim.x) {
    L.key[s] = -1;
    L.xmin[s] = L.ymin[s] = 0x7fffffff;
    L.xmax[s] = L.ymax[s] = -1;
    L.cnt[s] = 0;
  }
  __syncthreads();
  const long long n = (long long)H * W, groups = (n + INST_PX - 1) / INST_PX;
  const long long g0 = blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  bool bad = false;
  for (long long gb = g0; gb < g1; gb += blockDim.x) {         // the trip count is uniform over the workgroup
    const long long g = gb + threadIdx.x;
    const bool active = g < g1;
    const long long i0 = g * INST_PX;
    int k[INST_PX];
    if (active) {
      inst_load(inst, i0, n, vec != 0, [](T v) { return inst_id(v); }, k);
    } else {
#pragma unroll
      for (int j = 0; j < INST_PX; ++j) k[j] = -3;
    }
    bool same = true;
#pragma unroll
    for (int j = 0; j < INST_PX; ++j) {
      bad |= k[j] == -2;
      k[j] = k[j] >= min_id ? k[j] : -1;                       // below min_id, out of range, behind the end: no object
      same &= k[j] == k[0];
    }
    int x = active ? (int)(i0 % W) : 0, y = active ? (int)(i0 / W) : 0;
    same &= x + INST_PX <= W;                                  // one row
    const int first = __shfl(k[0], 0, 64);
    if (__all(same && k[0] >= 0 && k[0] == first)) {
      // the whole wave lies inside one object: one update for its 64 * INST_PX pixels
      const int x0 = inst_wave_min(x), x1 = inst_wave_max(x + INST_PX - 1), y0 = inst_wave_min(y), y1 = inst_wave_max(y);
      if ((threadIdx.x & 63) == 0) inst_box_add(L, box, k[0], x0, x1, y0, y1, 64 * INST_PX);
      continue;
    }
    int rk = -1, rx = 0, ry = 0, rn = 0;                       // the open run: key, first x, row, length
#pragma unroll
    for (int j = 0; j < INST_PX; ++j) {
      if (k[j] != rk || x == 0) {                              // a run ends with its key or with its row
        if (rk >= 0) inst_box_add(L, box, rk, rx, rx + rn - 1, ry, ry, rn);
        rk = k[j]; rx = x; ry = y; rn = 0;
      }
      ++rn;
      if (++x == W) { x = 0; ++y; }
    }
    if (rk >= 0) inst_box_add(L, box, rk, rx, rx + rn - 1, ry, ry, rn);
  }
  if (bad) atomicOr(&status[1], HIM_INST_ID_RANGE);
  __syncthreads();
  for (int s = threadIdx.x; s < INST_BOX_SLOTS; s += blockDim.x) {
    const int id = L.key[s];
    if (id < 0) continue;
    atomicMin(&box[id], L.xmin[s]);
    atomicMin(&box[INST_IDS + id], L.ymin[s]);
    atomicMax(&box[2 * INST_IDS + id], L.xmax[s]);
    atomicMax(&box[3 * INST_IDS + id], L.ymax[s]);
    atomicAdd(&box[4 * INST_IDS + id], L.cnt[s]);
  }
}

// One workgroup of 1024 threads, 64 ids each: the present ids in ascending order -> table rows and the id -> row map
__global__ __launch_bounds__(1024) void inst_compact_kernel(const int* __restrict__ box, int* __restrict__ rowmap,
                                                            int max_objects, int* __restrict__ status,
                                                            int* __restrict__ table) {
  __shared__ int wave_total[16];
  const int t = threadIdx.x, lane = t & 63;
  const int* cnt = box + 4 * INST_IDS;
  unsigned long long present = 0ull;
  int mine = 0;
  for (int j = 0; j < 64; ++j)
    if (cnt[t * 64 + j] > 0) { present |= 1ull << j; ++mine; }
  int inc = mine;                                              // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wave_total[t >> 6] = inc;
  __syncthreads();
  int row = inc - mine, total = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < (t >> 6)) row += wave_total[w];
    total += wave_total[w];
  }
  for (int j = 0; j < 64; ++j) {
    const int id = t * 64 + j;
    int r = -1;
    if ((present >> j) & 1ull) {
      if (row < max_objects) {
        r = row;
        int* o = table + (long long)r * 7;
        o[0] = id;
        o[1] = box[id];
        o[2] = box[INST_IDS + id];
        o[3] = box[2 * INST_IDS + id];
        o[4] = box[3 * INST_IDS + id];
        o[5] = cnt[id];
        o[6] = 0;
      }
      ++row;
    }
    rowmap[id] = r;
  }
  if (t == 0) {
    status[0] = total;
    if (total > max_objects) status[1] |= HIM_INST_OVERFLOW;
  }
}

struct InstClsLds {
  int key[INST_CLS_SLOTS], cnt[INST_CLS_SLOTS];
};

// key = id << 8 | class
__device__ __forceinline__ void inst_cls_add(InstClsLds& L, const int* __restrict__ rowmap, int* __restrict__ hist,
                                             int key, int n) {
  const int s = inst_slot<INST_CLS_SLOTS>(L.key, key);
  if (s >= 0) {
    atomicAdd(&L.cnt[s], n);
  } else {
    const int row = rowmap[key >> 8];
    if (row >= 0) atomicAdd(&hist[row * 256 + (key & 255)], n);
  }
}

template <typename T, typename C>
__global__ __launch_bounds__(256) void inst_class_kernel(const T* __restrict__ inst, const C* __restrict__ cls, int H,
                                                         int W, int vec, int min_id, long long per,
                                                         const int* __restrict__ rowmap, int* __restrict__ hist,
                                                         int* __restrict__ status) {
  __shared__ InstClsLds L;
  for (int s = threadIdx.x; s < INST_CLS_SLOTS; s += blockDim.x) {
    L.key[s] = -1;
    L.cnt[s] = 0;
  }
  __syncthreads();
  const long long n = (long long)H * W, groups = (n + INST_PX - 1) / INST_PX;
  const long long g0 = blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  bool bad = false;
  for (long long gb = g0; gb < g1; gb += blockDim.x) {
    const long long g = gb + threadIdx.x;
    const bool active = g < g1;
    const long long i0 = g * INST_PX;
    int k[INST_PX], c[INST_PX];
    if (active) {
      inst_load(inst, i0, n, vec != 0, [](T v) { return inst_id(v); }, k);
      inst_load(cls, i0, n, vec != 0, [](C v) { return inst_cls(v); }, c);
    } else {
#pragma unroll
      for (int j = 0; j < INST_PX; ++j) k[j] = c[j] = -3;
    }
    bool same = true;
#pragma unroll
    for (int j = 0; j < INST_PX; ++j) {
      bad |= c[j] == -2;
      k[j] = (k[j] >= min_id && c[j] >= 0) ? ((k[j] << 8) | c[j]) : -1;
      same &= k[j] == k[0];
    }
    const int first = __shfl(k[0], 0, 64);
    if (__all(same && k[0] >= 0 && k[0] == first)) {
      if ((threadIdx.x & 63) == 0) inst_cls_add(L, rowmap, hist, k[0], 64 * INST_PX);
      continue;
    }
    int rk = -1, rn = 0;
#pragma unroll
    for (int j = 0; j < INST_PX; ++j) {
      if (k[j] != rk) {
        if (rk >= 0) inst_cls_add(L, rowmap, hist, rk, rn);
        rk = k[j]; rn = 0;
      }
      ++rn;
    }
    if (rk >= 0) inst_cls_add(L, rowmap, hist, rk, rn);
  }
  if (bad) atomicOr(&status[1], HIM_INST_CLS_RANGE);
  __syncthreads();
  for (int s = threadIdx.x; s < INST_CLS_SLOTS; s += blockDim.x) {
    const int key = L.key[s];
    if (key < 0) continue;
    const int row = rowmap[key >> 8];
    if (row >= 0) atomicAdd(&hist[row * 256 + (key & 255)], L.cnt[s]);
  }
}

// one wave per table row: the two middle order statistics of its 256 bins, cls = (lo + hi) >> 1
__global__ __launch_bounds__(256) void inst_median_kernel(const int* __restrict__ hist, const int* __restrict__ status,
                                                          int max_objects, int* __restrict__ table) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int rows = status[0] < max_objects ? status[0] : max_objects;
  if (row >= rows) return;                                     // whole waves leave; no barrier below
  const int4 h = ((const int4*)(hist + row * 256))[lane];
  const int mine = h.x + h.y + h.z + h.w;
  int inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  const int n = table[row * 7 + 5], klo = (n - 1) >> 1, khi = n >> 1;
  const int bins[4] = {h.x, h.y, h.z, h.w};
  int lo = -1, hi = -1, before = inc - mine;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int upto = before + bins[q];
    if (klo >= before && klo < upto) lo = lane * 4 + q;
    if (khi >= before && khi < upto) hi = lane * 4 + q;
    before = upto;
  }
  lo = inst_wave_max(lo);
  hi = inst_wave_max(hi);
  if (lane == 0) table[row * 7 + 6] = (lo < 0 || hi < 0) ? 0 : (lo + hi) >> 1;   // not found: pixels outside the class domain
}

static inline size_t inst_ws_bytes(int max_objects) {
  return ((size_t)6 * INST_IDS + (size_t)max_objects * 256) * sizeof(int);
}
static inline bool inst_vec(const void* p, int W) { return W % INST_PX == 0 && (uintptr_t)p % 16 == 0; }

template <typename T>
static void inst_launch_class(const T* inst, const void* cls, int cls_kind, int H, int W, int vec, int min_id,
                              long long per, dim3 grid, const int* rowmap, int* hist, int* status, hipStream_t st) {
  switch (cls_kind) {
    case 0: hipLaunchKernelGGL((inst_class_kernel<T, unsigned char>), grid, dim3(256), 0, st, inst,
                               (const unsigned char*)cls, H, W, vec, min_id, per, rowmap, hist, status); break;
    case 1: hipLaunchKernelGGL((inst_class_kernel<T, int>), grid, dim3(256), 0, st, inst, (const int*)cls, H, W, vec,
                               min_id, per, rowmap, hist, status); break;
    case 2: hipLaunchKernelGGL((inst_class_kernel<T, long long>), grid, dim3(256), 0, st, inst, (const long long*)cls, H,
                               W, vec, min_id, per, rowmap, hist, status); break;
    default: hipLaunchKernelGGL((inst_class_kernel<T, float>), grid, dim3(256), 0, st, inst, (const float*)cls, H, W,
                                vec, min_id, per, rowmap, hist, status); break;
  }
}

// ---- ADE20K segmentation decode (reference preprocess_ade.py loadAde20K + the relabel / box loops of its main) ----------
// Three launches: setup (clear the 256 bins, build the class -> label table), first pass (classes, labels, the raw B
// plane and a box + count per B value), second pass (B values present -> ranks: table, status, the B plane mapped in
// place).  A lane owns ADE_PX adjacent pixels of the flattened image; on the vector path it reads them as whole 16-byte
// words (ADE_PX * pixel_bytes = 48 or 64 bytes) and stores each output as 16-byte words, on the element path byte by
// byte with a bound per pixel -- the same code behind both.  B runs are folded before they reach the 256 LDS bins, and a
// workgroup flushes only the bins it touched.  Integer min / max / add only.
#define ADE_PX 16
#define ADE_BINS 256
#define ADE_CLASSES 6656                                       // (255 / 10) * 256 + 255 + 1 raw class values
#define ADE_WS_BYTES ((size_t)5 * ADE_BINS * sizeof(int) + ADE_CLASSES)

struct AdeLds {
  alignas(16) unsigned char lut[ADE_CLASSES];
  int xmin[ADE_BINS], ymin[ADE_BINS], xmax[ADE_BINS], ymax[ADE_BINS], cnt[ADE_BINS];
};

// one workgroup: bins to their neutral values; lut[class] = 1-based position of its FIRST occurrence in keep, else 0
__global__ __launch_bounds__(256) void ade_setup_kernel(const unsigned short* __restrict__ keep, int n_keep,
                                                        int* __restrict__ bins, unsigned char* __restrict__ lut) {
  __shared__ alignas(16) unsigned char table[ADE_CLASSES];
  __shared__ unsigned short k[256];
  const int t = threadIdx.x;
  bins[t] = bins[ADE_BINS + t] = 0x7fffffff;
  bins[2 * ADE_BINS + t] = bins[3 * ADE_BINS + t] = -1;
  bins[4 * ADE_BINS + t] = 0;
  for (int i = t; i < ADE_CLASSES / 4; i += 256) ((unsigned*)table)[i] = 0u;
  k[t] = t < n_keep ? keep[t] : (unsigned short)0;
  __syncthreads();
  if (t < n_keep && k[t] < ADE_CLASSES) {
    bool first = true;
    for (int i = 0; i < t; ++i) first &= k[i] != k[t];
    if (first) table[k[t]] = (unsigned char)(t + 1);
  }
  __syncthreads();
  for (int i = t; i < ADE_CLASSES / 4; i += 256) ((unsigned*)lut)[i] = ((const unsigned*)table)[i];
}

__device__ __forceinline__ void ade_box_add(AdeLds& L, int b, int x0, int x1, int y0, int y1, int n) {
  atomicMin(&L.xmin[b], x0);
  atomicMin(&L.ymin[b], y0);
  atomicMax(&L.xmax[b], x1);
  atomicMax(&L.ymax[b], y1);
  atomicAdd(&L.cnt[b], n);
}

// workgroup b owns the groups [b * per, (b + 1) * per) of ADE_PX pixels; PB = bytes per pixel (3 or 4)
template <int PB>
__global__ __launch_bounds__(256) void ade_first_kernel(const unsigned char* __restrict__ seg, int H, int W, int vec,
                                                        long long per, const unsigned char* __restrict__ lut,
                                                        unsigned short* __restrict__ cls_out,
                                                        unsigned char* __restrict__ label_out,
                                                        unsigned char* __restrict__ inst_out, int* __restrict__ bins) {
  __shared__ AdeLds L;
  for (int i = threadIdx.x; i < ADE_CLASSES / 16; i += blockDim.x) ((uint4*)L.lut)[i] = ((const uint4*)lut)[i];
  for (int s = threadIdx.x; s < ADE_BINS; s += blockDim.x) {
    L.xmin[s] = L.ymin[s] = 0x7fffffff;
    L.xmax[s] = L.ymax[s] = -1;
    L.cnt[s] = 0;
  }
  __syncthreads();
  const long long n = (long long)H * W, groups = (n + ADE_PX - 1) / ADE_PX;
  const long long g0 = blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  struct alignas(16) In { unsigned char a[ADE_PX * PB]; };
  struct alignas(16) Out8 { unsigned char a[ADE_PX]; };
  struct alignas(16) Out16 { unsigned short a[ADE_PX]; };
  for (long long gb = g0; gb < g1; gb += blockDim.x) {         // the trip count is uniform over the workgroup
    const long long g = gb + threadIdx.x;
    const bool active = g < g1;
    const long long i0 = g * ADE_PX;
    const int m = !active ? 0 : (n - i0 < ADE_PX ? (int)(n - i0) : ADE_PX);      // pixels of this group inside the plane
    const bool whole = vec != 0 && m == ADE_PX;
    In in;
    if (whole) {
      in = *(const In*)(seg + i0 * PB);
    } else {
#pragma unroll
      for (int k = 0; k < ADE_PX; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) in.a[k * PB + c] = k < m ? seg[(i0 + k) * PB + c] : (unsigned char)0;
      }
    }
    Out16 oc;
    Out8 ol, ob;
#pragma unroll
    for (int k = 0; k < ADE_PX; ++k) {
      const int c = (in.a[k * PB] / 10) * 256 + in.a[k * PB + 1];
      oc.a[k] = (unsigned short)c;
      ol.a[k] = L.lut[c];
      ob.a[k] = in.a[k * PB + 2];
    }
    if (whole) {
      if (cls_out) *(Out16*)(cls_out + i0) = oc;
      *(Out8*)(label_out + i0) = ol;
      *(Out8*)(inst_out + i0) = ob;
    } else {
#pragma unroll
      for (int k = 0; k < ADE_PX; ++k) {
        if (k < m) {
          if (cls_out) cls_out[i0 + k] = oc.a[k];
          label_out[i0 + k] = ol.a[k];
          inst_out[i0 + k] = ob.a[k];
        }
      }
    }
    int x = active ? (int)(i0 % W) : 0, y = active ? (int)(i0 / W) : 0;
    bool same = m == ADE_PX && x + ADE_PX <= W;                // a whole group inside one row
#pragma unroll
    for (int k = 1; k < ADE_PX; ++k) same &= ob.a[k] == ob.a[0];
    const int first = __shfl((int)ob.a[0], 0, 64);
    if (__all(same && (int)ob.a[0] == first)) {
      // the whole wave lies inside one instance: one update for its 64 * ADE_PX pixels
      const int x0 = inst_wave_min(x), x1 = inst_wave_max(x + ADE_PX - 1), y0 = inst_wave_min(y), y1 = inst_wave_max(y);
      if ((threadIdx.x & 63) == 0) ade_box_add(L, first, x0, x1, y0, y1, 64 * ADE_PX);
      continue;
    }
    int rk = -1, rx = 0, ry = 0, rn = 0;                       // the open run: B value, first x, row, length
#pragma unroll
    for (int k = 0; k < ADE_PX; ++k) {
      if (k < m) {
        if ((int)ob.a[k] != rk || x == 0) {                    // a run ends with its value or with its row
          if (rk >= 0) ade_box_add(L, rk, rx, rx + rn - 1, ry, ry, rn);
          rk = ob.a[k]; rx = x; ry = y; rn = 0;
        }
        ++rn;
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (rk >= 0) ade_box_add(L, rk, rx, rx + rn - 1, ry, ry, rn);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < ADE_BINS; s += blockDim.x) {
    if (L.cnt[s] == 0) continue;                               // only the bins this workgroup touched
    atomicMin(&bins[s], L.xmin[s]);
    atomicMin(&bins[ADE_BINS + s], L.ymin[s]);
    atomicMax(&bins[2 * ADE_BINS + s], L.xmax[s]);
    atomicMax(&bins[3 * ADE_BINS + s], L.ymax[s]);
    atomicAdd(&bins[4 * ADE_BINS + s], L.cnt[s]);
  }
}

// Every workgroup ranks the 256 presence counts (thread t = B value t) and maps its share of the B plane in place;
// workgroup 0 also writes the table rows and the status record.
__global__ __launch_bounds__(256) void ade_rank_kernel(const int* __restrict__ bins, long long n, long long per, int vec,
                                                       unsigned char* __restrict__ inst_out, int* __restrict__ status,
                                                       int* __restrict__ table) {
  __shared__ unsigned char rank[ADE_BINS];
  __shared__ int wave_total[4];
  const int t = threadIdx.x, lane = t & 63;
  const int count = bins[4 * ADE_BINS + t];
  const unsigned long long present = __ballot(count > 0);
  if (lane == 0) wave_total[t >> 6] = __popcll(present);
  __syncthreads();
  int r = __popcll(present & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < (t >> 6)) r += wave_total[w];
    total += wave_total[w];
  }
  rank[t] = (unsigned char)r;                                  // read only where the value occurs
  if (blockIdx.x == 0) {
    if (count > 0) {
      int* o = table + r * 7;
      o[0] = r;
      o[1] = t;
      o[2] = bins[t];
      o[3] = bins[ADE_BINS + t];
      o[4] = bins[2 * ADE_BINS + t];
      o[5] = bins[3 * ADE_BINS + t];
      o[6] = count;
    }
    if (t == 0) {
      status[0] = total;
      status[1] = 0;
    }
  }
  __syncthreads();
  struct alignas(16) Q { unsigned char a[ADE_PX]; };
  const long long groups = (n + ADE_PX - 1) / ADE_PX;
  const long long g0 = blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  for (long long g = g0 + t; g < g1; g += blockDim.x) {
    const long long i0 = g * ADE_PX;
    if (vec != 0 && i0 + ADE_PX <= n) {
      Q q = *(const Q*)(inst_out + i0);
#pragma unroll
      for (int k = 0; k < ADE_PX; ++k) q.a[k] = rank[q.a[k]];
      *(Q*)(inst_out + i0) = q;
    } else {
      for (int k = 0; k < ADE_PX && i0 + k < n; ++k) inst_out[i0 + k] = rank[inst_out[i0 + k]];
    }
  }
}

}  // namespace him

using namespace him;
#define ST ((hipStream_t)stream)

extern "C" {

int him_data_nearest(const void* base, const long long* off, const int* pitch, const int* xtab, const int* ytab,
                     int src_kind, void* dst, int dst_kind, int B, int H, int W, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0) return fail(HIM_E_INVALID, "data_nearest: bad shape");
  if (dst_kind < 0 || dst_kind > 3) return fail(HIM_E_INVALID, "data_nearest: dst_kind %d", dst_kind);
  dim3 g = data_grid((long long)B * H * W);
  const unsigned char* p = (const unsigned char*)base;
  switch (src_kind) {
    case 0: hipLaunchKernelGGL(data_nearest_kernel<unsigned char>, g, dim3(256), 0, ST, p, off, pitch, xtab, ytab, dst,
                               dst_kind, B, H, W); break;
    case 1: hipLaunchKernelGGL(data_nearest_kernel<unsigned short>, g, dim3(256), 0, ST, p, off, pitch, xtab, ytab, dst,
                               dst_kind, B, H, W); break;
    case 2: hipLaunchKernelGGL(data_nearest_kernel<int>, g, dim3(256), 0, ST, p, off, pitch, xtab, ytab, dst, dst_kind,
                               B, H, W); break;
    default: return fail(HIM_E_INVALID, "data_nearest: src_kind %d", src_kind);
  }
  return check_launch("data_nearest");
}

int him_data_nearest_rle(const void* base, const long long* row_off, const long long* runx_off,
                         const long long* runv_off, const int* x0, const int* y0, const int* xtab, const int* ytab,
                         void* dst, int dst_kind, int B, int H, int W, void* stream) {
  if (!base || !row_off || !runx_off || !runv_off || !x0 || !y0 || !xtab || !ytab || !dst)
    return fail(HIM_E_INVALID, "data_nearest_rle: null pointer");
  if (B <= 0 || H <= 0 || W <= 0) return fail(HIM_E_INVALID, "data_nearest_rle: bad shape");
  if (dst_kind < 0 || dst_kind > 3) return fail(HIM_E_INVALID, "data_nearest_rle: dst_kind %d", dst_kind);
  const size_t elem = dst_kind == 2 ? 1 : 4;
  const int vec = W % RLE_PX == 0 && (uintptr_t)dst % (RLE_PX * elem) == 0;
  const long long groups = (long long)B * H * ((W + RLE_PX - 1) / RLE_PX);
  hipLaunchKernelGGL(data_nearest_rle_kernel, data_grid(groups), dim3(256), 0, ST, (const unsigned char*)base, row_off,
                     runx_off, runv_off, x0, y0, xtab, ytab, dst, dst_kind, vec, B, H, W);
  return check_launch("data_nearest_rle");
}

int him_data_bicubic_h(const void* base, const long long* off, const int* pitch, const int* rows, const int* first,
                       const int* count, const int* weights, int ksize, unsigned char* tmp, int maxrows, int B, int W,
                       void* stream) {
  if (B <= 0 || W <= 0 || maxrows <= 0 || ksize <= 0 || maxrows > 65535 || B > 65535)
    return fail(HIM_E_INVALID, "data_bicubic_h: bad shape");
  hipLaunchKernelGGL(data_bicubic_h_kernel, dim3((W + 255) / 256, maxrows, B), dim3(256), 0, ST,
                     (const unsigned char*)base, off, pitch, rows, first, count, weights, ksize, tmp, maxrows, B, W);
  return check_launch("data_bicubic_h");
}

int him_data_bicubic_v(const unsigned char* tmp, int maxrows, const int* first, const int* count, const int* weights,
                       int ksize, const int* flip, float* dst, int normalize, int B, int H, int W, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || ksize <= 0 || H > 65535 || B > 65535)
    return fail(HIM_E_INVALID, "data_bicubic_v: bad shape");
  hipLaunchKernelGGL(data_bicubic_v_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, ST, tmp, maxrows, first, count,
                     weights, ksize, flip, dst, normalize, B, H, W);
  return check_launch("data_bicubic_v");
}

int him_data_region_masks(const float* label, const void* inst, int inst_kind, const int* boxes, const float* fill,
                          const int* inst_id, float* mask_in, float* obj_in, float* ctx_in, float* mask_out,
                          float* obj_out, float* inst_mask, int B, int H, int W, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0) return fail(HIM_E_INVALID, "data_region_masks: bad shape");
  if (inst_mask && (!inst || !inst_id)) return fail(HIM_E_INVALID, "data_region_masks: instance mask without a map");
  hipLaunchKernelGGL(data_region_masks_kernel, data_grid((long long)B * H * W), dim3(256), 0, ST, label, inst,
                     inst_kind, boxes, fill, inst_id, mask_in, obj_in, ctx_in, mask_out, obj_out, inst_mask, B, H, W);
  return check_launch("data_region_masks");
}

int him_canvas_window_bytes(const float* src, int C, int Hs, int Ws, int x0, int y0, int h, int w, int pre,
                            unsigned char* dst, void* stream) {
  if (C <= 0 || Hs <= 0 || Ws <= 0 || h <= 0 || w <= 0) return fail(HIM_E_INVALID, "canvas_window_bytes: bad shape");
  if (pre < 0 || pre > 2) return fail(HIM_E_INVALID, "canvas_window_bytes: pre %d", pre);
  hipLaunchKernelGGL(canvas_window_bytes_kernel, data_grid((long long)h * w), dim3(256), 0, ST, src, C, Hs, Ws, x0, y0, h,
                     w, pre, dst);
  return check_launch("canvas_window_bytes");
}

int him_canvas_paste_bicubic_v(const unsigned char* tmp, const int* first, const int* count, const int* weights,
                               int ksize, float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, void* stream) {
  if (H <= 0 || W <= 0 || ksize <= 0 || H > 65535) return fail(HIM_E_INVALID, "canvas_paste_bicubic_v: bad shape");
  if (x0 < 0 || y0 < 0 || x0 + W > Wc || y0 + H > Hc)
    return fail(HIM_E_INVALID, "canvas_paste_bicubic_v: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, W, H,
                Wc, Hc);
  hipLaunchKernelGGL(canvas_paste_bicubic_v_kernel, dim3((W + 255) / 256, H), dim3(256), 0, ST, tmp, first, count,
                     weights, ksize, canvas, Hc, Wc, x0, y0, W);
  return check_launch("canvas_paste_bicubic_v");
}

int him_canvas_paste_window(const void* src, int src_kind, int C, int h, int w, float* canvas, int Hc, int Wc, int x0,
                            int y0, void* stream) {
  if (C <= 0 || h <= 0 || w <= 0) return fail(HIM_E_INVALID, "canvas_paste_window: bad shape");
  if (src_kind < 0 || src_kind > 1) return fail(HIM_E_INVALID, "canvas_paste_window: src_kind %d", src_kind);
  if (x0 < 0 || y0 < 0 || x0 + w > Wc || y0 + h > Hc)
    return fail(HIM_E_INVALID, "canvas_paste_window: window (%d,%d)+(%d,%d) outside the %dx%d canvas", x0, y0, w, h, Wc,
                Hc);
  hipLaunchKernelGGL(canvas_paste_window_kernel, data_grid((long long)C * h * w), dim3(256), 0, ST, src, src_kind, C, h,
                     w, canvas, Hc, Wc, x0, y0);
  return check_launch("canvas_paste_window");
}

int him_tensor2im_bytes(const float* src, int C, int H, int W, int normalize, unsigned char* dst, void* stream) {
  if (H <= 0 || W <= 0) return fail(HIM_E_INVALID, "tensor2im_bytes: bad shape");
  if (C != 1 && C != 3) return fail(HIM_E_INVALID, "tensor2im_bytes: %d channels (1 or 3)", C);
  if (!src || !dst) return fail(HIM_E_INVALID, "tensor2im_bytes: null pointer");
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(tensor2im_bytes_kernel, vis_grid(n), dim3(256), 0, ST, src, C, n, normalize ? 1 : 0,
                     vis_vec(src, n, sizeof(float)) ? 1 : 0, vis_packed(dst) ? 1 : 0, dst);
  return check_launch("tensor2im_bytes");
}

int him_label2color_bytes(const void* src, int dtype, int C, int H, int W, const unsigned char* table, int n,
                          unsigned char* dst, void* stream) {
  if (C <= 0 || H <= 0 || W <= 0) return fail(HIM_E_INVALID, "label2color_bytes: bad shape");
  if (n <= 0 || n > 8192) return fail(HIM_E_INVALID, "label2color_bytes: %d table rows (1..8192)", n);
  if (!src || !table || !dst) return fail(HIM_E_INVALID, "label2color_bytes: null pointer");
  if (C > 1 && dtype != 0) return fail(HIM_E_INVALID, "label2color_bytes: scores are fp32 (dtype %d)", dtype);
  const long long px = (long long)H * W;
  const dim3 g = vis_grid(px);
  const size_t lds = (size_t)n * sizeof(unsigned);
  const int packed = vis_packed(dst) ? 1 : 0;
  switch (dtype) {
    case 0: hipLaunchKernelGGL(label2color_bytes_kernel<float>, g, dim3(256), lds, ST, (const float*)src, C, px, table, n,
                               vis_vec(src, px, sizeof(float)) ? 1 : 0, packed, dst); break;
    case 1: hipLaunchKernelGGL(label2color_bytes_kernel<unsigned char>, g, dim3(256), lds, ST, (const unsigned char*)src,
                               C, px, table, n, vis_vec(src, px, 1) ? 1 : 0, packed, dst); break;
    case 2: hipLaunchKernelGGL(label2color_bytes_kernel<long long>, g, dim3(256), lds, ST, (const long long*)src, C, px,
                               table, n, vis_vec(src, px, sizeof(long long)) ? 1 : 0, packed, dst); break;
    default: return fail(HIM_E_INVALID, "label2color_bytes: dtype %d", dtype);
  }
  return check_launch("label2color_bytes");
}

int him_seglabel_bytes(const float* src, int C, int H, int W, unsigned char* dst, void* stream) {
  if (C <= 0 || H <= 0 || W <= 0) return fail(HIM_E_INVALID, "seglabel_bytes: bad shape");
  if (!src || !dst) return fail(HIM_E_INVALID, "seglabel_bytes: null pointer");
  const long long n = (long long)H * W;
  const dim3 g = vis_grid(n);
  const int vec = vis_vec(src, n, sizeof(float)) ? 1 : 0, packed = vis_packed(dst) ? 1 : 0;
  switch (C) {
    case 1: hipLaunchKernelGGL(seglabel_bytes_kernel<1>, g, dim3(256), 0, ST, src, C, n, vec, packed, dst); break;
    case 2: hipLaunchKernelGGL(seglabel_bytes_kernel<2>, g, dim3(256), 0, ST, src, C, n, vec, packed, dst); break;
    case 3: hipLaunchKernelGGL(seglabel_bytes_kernel<3>, g, dim3(256), 0, ST, src, C, n, vec, packed, dst); break;
    case 4: hipLaunchKernelGGL(seglabel_bytes_kernel<4>, g, dim3(256), 0, ST, src, C, n, vec, packed, dst); break;
    default: hipLaunchKernelGGL(seglabel_bytes_kernel<0>, g, dim3(256), 0, ST, src, C, n, vec, packed, dst); break;
  }
  return check_launch("seglabel_bytes");
}

size_t him_inst_summary_workspace(int H, int W, int max_objects) {
  if (H <= 0 || W <= 0 || max_objects <= 0 || max_objects > INST_IDS) return 0;
  return inst_ws_bytes(max_objects);
}

int him_inst_summary(const void* inst, int inst_kind, const void* cls, int cls_kind, int H, int W, int min_id,
                     int max_objects, int* status, int* table, void* ws, size_t ws_bytes, void* stream) {
  if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return fail(HIM_E_INVALID, "inst_summary: bad shape");
  if (max_objects <= 0 || max_objects > INST_IDS)
    return fail(HIM_E_INVALID, "inst_summary: max_objects %d (1..%d)", max_objects, INST_IDS);
  if (!inst || !cls || !status || !table || !ws) return fail(HIM_E_INVALID, "inst_summary: null pointer");
  if (inst_kind < 0 || inst_kind > 3) return fail(HIM_E_INVALID, "inst_summary: inst_kind %d", inst_kind);
  if (cls_kind < 0 || cls_kind > 3) return fail(HIM_E_INVALID, "inst_summary: cls_kind %d", cls_kind);
  if ((uintptr_t)ws % 16 != 0) return fail(HIM_E_INVALID, "inst_summary: workspace not 16-byte aligned");
  if (ws_bytes < inst_ws_bytes(max_objects))
    return fail(HIM_E_INVALID, "inst_summary: workspace %zu < %zu bytes", ws_bytes, inst_ws_bytes(max_objects));
  if (min_id < 0) min_id = 0;
  int* box = (int*)ws;
  int* rowmap = box + 5 * INST_IDS;
  int* hist = box + 6 * INST_IDS;
  const long long groups = ((long long)H * W + INST_PX - 1) / INST_PX;
  long long blocks = (groups + 511) / 512;
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  const long long per = (groups + blocks - 1) / blocks;
  const dim3 grid((unsigned)blocks);
  const int nhist = max_objects * 256;
  hipLaunchKernelGGL(inst_clear_kernel, data_grid(5 * INST_IDS + (long long)nhist), dim3(256), 0, ST, box, nhist, status);
  const int bvec = inst_vec(inst, W) ? 1 : 0, cvec = (bvec && inst_vec(cls, W)) ? 1 : 0;
  switch (inst_kind) {
    case 0: hipLaunchKernelGGL(inst_box_kernel<unsigned char>, grid, dim3(256), 0, ST, (const unsigned char*)inst, H, W,
                               bvec, min_id, per, box, status); break;
    case 1: hipLaunchKernelGGL(inst_box_kernel<unsigned short>, grid, dim3(256), 0, ST, (const unsigned short*)inst, H, W,
                               bvec, min_id, per, box, status); break;
    case 2: hipLaunchKernelGGL(inst_box_kernel<int>, grid, dim3(256), 0, ST, (const int*)inst, H, W, bvec, min_id, per,
                               box, status); break;
    default: hipLaunchKernelGGL(inst_box_kernel<long long>, grid, dim3(256), 0, ST, (const long long*)inst, H, W, bvec,
                                min_id, per, box, status); break;
  }
  hipLaunchKernelGGL(inst_compact_kernel, dim3(1), dim3(1024), 0, ST, box, rowmap, max_objects, status, table);
  switch (inst_kind) {
    case 0: inst_launch_class((const unsigned char*)inst, cls, cls_kind, H, W, cvec, min_id, per, grid, rowmap, hist,
                              status, ST); break;
    case 1: inst_launch_class((const unsigned short*)inst, cls, cls_kind, H, W, cvec, min_id, per, grid, rowmap, hist,
                              status, ST); break;
    case 2: inst_launch_class((const int*)inst, cls, cls_kind, H, W, cvec, min_id, per, grid, rowmap, hist, status, ST);
      break;
    default: inst_launch_class((const long long*)inst, cls, cls_kind, H, W, cvec, min_id, per, grid, rowmap, hist,
                               status, ST); break;
  }
  hipLaunchKernelGGL(inst_median_kernel, dim3((max_objects + 3) / 4), dim3(256), 0, ST, hist, status, max_objects, table);
  return check_launch("inst_summary");
}

size_t him_ade_decode_workspace(void) { return ADE_WS_BYTES; }

int him_ade_decode(const unsigned char* seg, int H, int W, int pixel_bytes, const unsigned short* keep, int n_keep,
                   unsigned short* cls_out, unsigned char* label_out, unsigned char* inst_out, int* status, int* table,
                   void* ws, size_t ws_bytes, void* stream) {
  if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return fail(HIM_E_INVALID, "ade_decode: bad shape");
  if (pixel_bytes != 3 && pixel_bytes != 4)
    return fail(HIM_E_INVALID, "ade_decode: pixel_bytes %d (3 or 4)", pixel_bytes);
  if (n_keep < 0 || n_keep > 255) return fail(HIM_E_INVALID, "ade_decode: n_keep %d (0..255)", n_keep);
  if (!seg || (!keep && n_keep > 0) || !label_out || !inst_out || !status || !table || !ws)
    return fail(HIM_E_INVALID, "ade_decode: null pointer");
  if ((uintptr_t)ws % 16 != 0) return fail(HIM_E_INVALID, "ade_decode: workspace not 16-byte aligned");
  if (ws_bytes < ADE_WS_BYTES)
    return fail(HIM_E_INVALID, "ade_decode: workspace %zu < %zu bytes", ws_bytes, (size_t)ADE_WS_BYTES);
  int* bins = (int*)ws;
  unsigned char* lut = (unsigned char*)(bins + 5 * ADE_BINS);
  const long long n = (long long)H * W, groups = (n + ADE_PX - 1) / ADE_PX;
  long long blocks = (groups + 511) / 512;
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  const long long per = (groups + blocks - 1) / blocks;
  const dim3 grid((unsigned)blocks);
  // whole 16-byte words need every plane's base on a 16-byte boundary (groups are 48 / 64 bytes in, 16 / 32 bytes out)
  const int vec = ((uintptr_t)seg % 16 == 0 && (uintptr_t)label_out % 16 == 0 && (uintptr_t)inst_out % 16 == 0 &&
                   (uintptr_t)cls_out % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(ade_setup_kernel, dim3(1), dim3(256), 0, ST, keep, n_keep, bins, lut);
  if (pixel_bytes == 3)
    hipLaunchKernelGGL(ade_first_kernel<3>, grid, dim3(256), 0, ST, seg, H, W, vec, per, lut, cls_out, label_out,
                       inst_out, bins);
  else
    hipLaunchKernelGGL(ade_first_kernel<4>, grid, dim3(256), 0, ST, seg, H, W, vec, per, lut, cls_out, label_out,
                       inst_out, bins);
  hipLaunchKernelGGL(ade_rank_kernel, grid, dim3(256), 0, ST, bins, n, per, vec, inst_out, status, table);
  return check_launch("ade_decode");
}

}  // extern "C"
