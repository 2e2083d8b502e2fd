// -*- c++ -*-
// Weight-gradient kernels (included by him_conv.hip inside namespace him): generic and fast MFMA split-K kernels with
// their fixed-order finish passes, the tiny-M VALU kernels, bias gradients; the few-channel MFMA kernel lives in
// him_wgrad_fewch.inc.
// ==============================================================================================
// wgrad
// ==============================================================================================
struct WGradP {
  const float* dy;  // [B][M][OH][OW]
  const float* x;   // [B][C][H][W]
  float* out;       // dW [M][Np]  or slabs [splits][M][Np]
  int M, C, B, H, W, OH, OW, KH, KW, stride, pad, pad_mode;
  int Np, Kdim, kchunk, splits, accumulate;
  FastDiv fKK, fKW, fOW;
};

template <int WM, int WN, int TM, int TN, bool REFLECT>
__global__ __launch_bounds__(256) void wgrad_kernel(const WGradP p) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, BK = 32;
  constexpr int LD = BK + 1;
  constexpr int RA = BM / 8, RB = BN / 8;
  static_assert(WM * WN == 4, "4 waves");
  __shared__ float sA[2][BM * LD];
  __shared__ float sB[2][BN * LD];
  __shared__ int tabOff[BN];
  __shared__ int tabD[BN];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int OHW = p.OH * p.OW, HW = p.H * p.W;
  const int kbeg = blockIdx.z * p.kchunk;
  const int kend = min(p.Kdim, kbeg + p.kchunk);

  // per-column (ci,kh,kw) table: loop invariant
  if (t < BN) {
    const int np = n0 + t;
    int off = 0, d = (128 << 16) | 128;
    if (np < p.Np) {
      const int ci = (int)fdiv((uint32_t)np, p.fKK);
      const int r = np - ci * p.KH * p.KW;
      const int kh = (int)fdiv((uint32_t)r, p.fKW);
      const int kw = r - kh * p.KW;
      off = ci * HW;
      d = ((kh - p.pad + 128) << 16) | (kw - p.pad + 128);
    }
    tabOff[t] = off;
    tabD[t] = d;
  }
  __syncthreads();

  const int kkl = t & 31, rg = t >> 5;
  // position of this thread's k index (b, sp) tracked incrementally
  int kcur = kbeg + kkl;
  int b = kcur / OHW;
  int sp = kcur - b * OHW;

  float ra[RA], rb[RB];
  const int H = p.H, W = p.W, stride = p.stride;
  const float* __restrict__ dy = p.dy;
  const float* __restrict__ x = p.x;
  uint32_t mrow[RA];
#pragma unroll
  for (int i = 0; i < RA; ++i) mrow[i] = (uint32_t)min(m0 + rg + 8 * i, p.M - 1) * (uint32_t)OHW;

  // branch-free: out-of-range k positions are redirected to element (0,0) and their dY operand zeroed;
  // out-of-range rows/columns are clamped and never stored.
  auto loadAB = [&]() {
    const bool kvalid = kcur < kend;
    const int bb = kvalid ? b : 0;
    const int spp = kvalid ? sp : 0;
    const int oh = (int)fdiv((uint32_t)spp, p.fOW);
    const int ow = spp - oh * p.OW;
    const uint32_t dyb = (uint32_t)bb * (uint32_t)p.M * (uint32_t)OHW + (uint32_t)spp;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      const float v = dy[dyb + mrow[i]];
      ra[i] = kvalid ? v : 0.f;
    }
    const uint32_t xb = (uint32_t)bb * (uint32_t)p.C * (uint32_t)HW;
    const int ihb = oh * stride, iwb = ow * stride;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int row = rg + 8 * i;
      const int off = tabOff[row];
      const int d = tabD[row];
      int ih = ihb + (d >> 16) - 128, iw = iwb + (d & 0xffff) - 128;
      bool ok = true;
      if (REFLECT) {
        ih = ih < 0 ? -ih : ih;
        ih = ih >= H ? 2 * (H - 1) - ih : ih;
        iw = iw < 0 ? -iw : iw;
        iw = iw >= W ? 2 * (W - 1) - iw : iw;
      } else {
        const int ch = min(max(ih, 0), H - 1), cw = min(max(iw, 0), W - 1);
        ok = (ch == ih) && (cw == iw);
        ih = ch;
        iw = cw;
      }
      const float v = x[xb + (uint32_t)off + (uint32_t)ih * (uint32_t)W + (uint32_t)iw];
      rb[i] = ok ? v : 0.f;
    }
  };
  auto advance = [&]() {
    kcur += BK;
    sp += BK;
    while (sp >= OHW) {
      sp -= OHW;
      ++b;
    }
  };
  auto storeAB = [&](int buf) {
#pragma unroll
    for (int i = 0; i < RA; ++i) sA[buf][(rg + 8 * i) * LD + kkl] = ra[i];
#pragma unroll
    for (int i = 0; i < RB; ++i) sB[buf][(rg + 8 * i) * LD + kkl] = rb[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, lh = lane >> 5;
  const int nk = (kend - kbeg + BK - 1) / BK;
  if (nk > 0) {
    loadAB();
    storeAB(0);
    advance();
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    loadAB();  // past the end: kvalid is false, loads hit element (0,0)
    const float* __restrict__ pa = &sA[buf][(wm * TM * 32 + l31) * LD + lh];
    const float* __restrict__ pb = &sB[buf][(wn * TN * 32 + l31) * LD + lh];
#pragma unroll
    for (int kp = 0; kp < BK / 2; ++kp) {
      float af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = pa[i * 32 * LD + kp * 2];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = pb[j * 32 * LD + kp * 2];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    storeAB(buf ^ 1);
    advance();
    __syncthreads();
  }

  float* __restrict__ out = p.out + (p.splits > 1 ? (size_t)blockIdx.z * p.M * p.Np : (size_t)0);
  const bool accum = p.splits == 1 && p.accumulate;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int np = n0 + wn * TN * 32 + j * 32 + l31;
    if (np >= p.Np) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < p.M) {
          float* o = out + (size_t)m * p.Np + np;
          *o = accum ? (*o + acc[i][j][r]) : acc[i][j][r];
        }
      }
    }
  }
}

// =============================================================================================
// wgrad, fast path (C % 64 == 0, OH*OW % 4 == 0): the filter-column index runs TAP-MAJOR, n' = tap*C + ci, so a
// 64/128-column tile is ONE filter tap x consecutive input channels: the gather coordinates (ih, iw, validity) are
// computed once per K-step per thread and every element is one saddr global_load.  dY tiles are contiguous float4s.
// LDS rows are [row][32 k + 4 pad] with the k <-> (lane>>5) pairing k = 16*(lane>>5) + kp (4 aligned ds_read_b128 per
// operand tile per K-step).  Partial results go to tap-major slabs; wgrad_finish_kernel sums the split-K slabs in
// fixed order and scatters into the reference (Cout,Cin,KH,KW) layout (+= for the gradient arena).
// =============================================================================================
#ifndef HIM_WG_DBG
#define HIM_WG_DBG 0   // tools/micro/wgrad_micro only (timing, wrong results): 1 no gathered loads, 2 no dY loads, 4 no LDS writes, 8 no MFMAs
#endif
template <int TM, int TN, bool REFLECT, bool AL4>
__global__ __launch_bounds__(256) void wgrad_fast_kernel(const WGradP p) {
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32, BK = 32, LD = 36;
  constexpr int A_V4 = BM * BK / 4 / 256;  // 4 or 2
  constexpr int RB = BN / 8;               // gathered rows per thread (16 or 8)
  __shared__ __attribute__((aligned(16))) float sA[2][BM * LD];
  __shared__ __attribute__((aligned(16))) float sB[2][BN * LD];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int OHW = p.OH * p.OW, HW = p.H * p.W, C = p.C;
  const int kbeg = blockIdx.z * p.kchunk;
  const int kend = min(p.Kdim, kbeg + p.kchunk);
  const int nk = (kend - kbeg + BK - 1) / BK;
  // the tile's filter tap (wave-uniform) and first input channel
  const int tap = n0 / C, ci0 = n0 - tap * C;
  const int th = tap / p.KW, tw = tap - th * p.KW;
  const int dh = th - p.pad, dw = tw - p.pad;
  const int H = p.H, W = p.W, stride = p.stride;

  // dY tile: thread -> (row = t/8 + 32 i, k quad = t%8)
  const int arow = t >> 3, akq = t & 7;
  uint32_t arowoff[A_V4];
#pragma unroll
  for (int i = 0; i < A_V4; ++i) arowoff[i] = (uint32_t)min(m0 + arow + 32 * i, p.M - 1) * (uint32_t)OHW;
  // gathered tile: thread -> (k = t%32, row group rg = t/32; rows rg + 8 i)
  const int kkl = t & 31, rg = t >> 5;

  // Both operands are read through BUFFER resources: an invalid element (K tail beyond kend, zero-padding tap) gets
  // voffset 0x80000000 and the range check returns 0.0 -- no select sits between a load and its ds_write, so nothing
  // makes the compiler wait for a load before the K-step's MFMAs have run (run_wgrad guarantees both tensors < 2 GiB).
  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.dy, 0, (int)((uint32_t)p.B * (uint32_t)p.M * (uint32_t)OHW * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.x, 0, (int)((uint32_t)p.B * (uint32_t)C * (uint32_t)HW * 4u), 0x00020000);
  const uint32_t xbase = (uint32_t)ci0 * (uint32_t)HW * 4u;   // wave-uniform: first channel of the tile
  const uint32_t step8 = 8u * (uint32_t)HW * 4u;

  // TWO register sets (round 5): the loads of tile kt+2 are issued at the top of K-step kt and stay in flight through all of
  // K-step kt+1 (one K-step of MFMAs did not cover the gathers: without any load the loop runs 17-27 % faster, tools/micro/
  // wgrad_micro -DHIM_WG_DBG=3); tile t travels in set X (t even) / Y (t odd)
  float4 raX[A_V4], raY[A_V4];
  float rbX[RB], rbY[RB];
  // per-thread cursors of the NEXT tile: A quad position and gather position, as (image, offset in image)
  int ka = kbeg + akq * 4, ba = ka / OHW, spa = ka - ba * OHW;
  int kb = kbeg + kkl, bb = kb / OHW, spb = kb - bb * OHW;

#define HIM_WLOAD(ra, rb)                                                                                         \
  {                                                                                                           \
    if (HIM_WG_DBG & 2) {                                                                                     \
      _Pragma("unroll") for (int i = 0; i < A_V4; ++i) ra[i] = make_float4(1.f, 1.f, 1.f, 1.f);               \
    } else if (AL4) {                                                                                         \
      const bool av = ka < kend;                                                                              \
      const uint32_t abase = (uint32_t)ba * (uint32_t)p.M * (uint32_t)OHW + (uint32_t)spa;                     \
      _Pragma("unroll") for (int i = 0; i < A_V4; ++i) {                                                      \
        ra[i] = __builtin_bit_cast(                                                                            \
            float4, __builtin_amdgcn_raw_buffer_load_b128(rdy, av ? (abase + arowoff[i]) * 4u : 0x80000000u, 0, 0)); \
      }                                                                                                       \
    } else { /* plane size not a multiple of 4 (odd PatchGAN planes): a quad may straddle two images */        \
      uint32_t eo[4];                                                                                         \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                         \
        int sp_ = spa + j, b_ = ba;                                                                           \
        const bool wrap = sp_ >= OHW;                                                                         \
        sp_ -= wrap ? OHW : 0;                                                                                \
        b_ += wrap ? 1 : 0;                                                                                   \
        eo[j] = (ka + j < kend) ? ((uint32_t)b_ * (uint32_t)p.M * (uint32_t)OHW + (uint32_t)sp_) * 4u : 0x80000000u; \
      }                                                                                                       \
      _Pragma("unroll") for (int i = 0; i < A_V4; ++i) {                                                      \
        float q_[4];                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                         \
          q_[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(                              \
              rdy, eo[j] == 0x80000000u ? eo[j] : eo[j] + arowoff[i] * 4u, 0, 0));                             \
        ra[i] = make_float4(q_[0], q_[1], q_[2], q_[3]);                                                      \
      }                                                                                                       \
    }                                                                                                         \
    const bool bv = kb < kend;                                                                                \
    const int sp = bv ? spb : 0;                                                                              \
    const int oh = (int)fdiv((uint32_t)sp, p.fOW);                                                            \
    const int ow = sp - oh * p.OW;                                                                            \
    int ih = oh * stride + dh, iw = ow * stride + dw;                                                         \
    bool ok = bv;                                                                                             \
    if (REFLECT) {                                                                                            \
      ih = ih < 0 ? -ih : ih;                                                                                 \
      ih = ih >= H ? 2 * (H - 1) - ih : ih;                                                                   \
      iw = iw < 0 ? -iw : iw;                                                                                 \
      iw = iw >= W ? 2 * (W - 1) - iw : iw;                                                                   \
    } else {                                                                                                  \
      ok = ok && ih >= 0 && ih < H && iw >= 0 && iw < W;                                                      \
    }                                                                                                         \
    const uint32_t voff = ok ? ((uint32_t)bb * (uint32_t)C * (uint32_t)HW + (uint32_t)rg * (uint32_t)HW +      \
                                (uint32_t)ih * (uint32_t)W + (uint32_t)iw) * 4u : 0x80000000u;                 \
    uint32_t so8 = xbase;                                                                                     \
    _Pragma("unroll") for (int i = 0; i < RB; ++i) {                                                          \
      rb[i] = (HIM_WG_DBG & 1) ? __builtin_bit_cast(float, voff)                                              \
                               : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff, so8, 0)); \
      so8 += step8;                                                                                           \
    }                                                                                                         \
    ka += BK;                                                                                                 \
    spa += BK;                                                                                                \
    while (spa >= OHW) {                                                                                      \
      spa -= OHW;                                                                                             \
      ++ba;                                                                                                   \
    }                                                                                                         \
    kb += BK;                                                                                                 \
    spb += BK;                                                                                                \
    while (spb >= OHW) {                                                                                      \
      spb -= OHW;                                                                                             \
      ++bb;                                                                                                   \
    }                                                                                                         \
  }
#define HIM_WSTORE(buf_, ra, rb)                                                                                     \
  if (!(HIM_WG_DBG & 4)) {                                                                                    \
    _Pragma("unroll") for (int i = 0; i < A_V4; ++i) *(float4*)&sA[buf_][(arow + 32 * i) * LD + akq * 4] = ra[i]; \
    _Pragma("unroll") for (int i = 0; i < RB; ++i) sB[buf_][(rg + 8 * i) * LD + kkl] = rb[i];                 \
  } else {                                                                                                    \
    float sink_ = 0.f;                                                                                        \
    _Pragma("unroll") for (int i = 0; i < A_V4; ++i) sink_ += ra[i].x + ra[i].y + ra[i].z + ra[i].w;          \
    _Pragma("unroll") for (int i = 0; i < RB; ++i) sink_ += rb[i];                                            \
    if (sink_ == 1.2345e-30f) sB[buf_][0] = sink_;                                                            \
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, lh = lane >> 5;
  if (nk > 0) {
    HIM_WLOAD(raX, rbX)
    HIM_WSTORE(0, raX, rbX)
    HIM_WLOAD(raY, rbY)   // tile 1 (past the end: zeros): in flight across the first K-step
  }
  __syncthreads();
#define HIM_WM(Q, CMP)                                                                                         \
  _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) {              \
    if (HIM_WG_DBG & 8) acc[i][j][0] += af[i][Q].CMP * bf[j][Q].CMP;                                          \
    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][Q].CMP, bf[j][Q].CMP, acc[i][j], 0, 0, 0);     \
  }
#define HIM_WKSTEP(kt_, LA, LB, SA, SB)                                                                         \
  {                                                                                                           \
    const int buf = (kt_) & 1;                                                     \
                                                                                                              \
    const float4* __restrict__ pa = (const float4*)&sA[buf][(wm * TM * 32 + l31) * LD + lh * 16];             \
    const float4* __restrict__ pb = (const float4*)&sB[buf][(wn * TN * 32 + l31) * LD + lh * 16];             \
    float4 af[TM][4], bf[TN][4];                                                                              \
_Pragma("unroll")                                                                                             \
    for (int i = 0; i < TM; ++i)                                                                              \
_Pragma("unroll")                                                                                             \
      for (int q = 0; q < 4; ++q) af[i][q] = pa[i * 32 * LD / 4 + q];                                         \
_Pragma("unroll")                                                                                             \
    for (int j = 0; j < TN; ++j)                                                                              \
_Pragma("unroll")                                                                                             \
      for (int q = 0; q < 4; ++q) bf[j][q] = pb[j * 32 * LD / 4 + q];                                         \
    HIM_WLOAD(LA, LB)  /* tile kt+2; past the end: both operands' validity is false -> zeros */               \
    HIM_WM(0, x) HIM_WM(0, y) HIM_WM(0, z) HIM_WM(0, w)                                                       \
    HIM_WM(1, x) HIM_WM(1, y) HIM_WM(1, z) HIM_WM(1, w)                                                       \
    HIM_WM(2, x) HIM_WM(2, y) HIM_WM(2, z) HIM_WM(2, w)                                                       \
    HIM_WM(3, x) HIM_WM(3, y) HIM_WM(3, z) HIM_WM(3, w)                                                       \
    HIM_WSTORE(buf ^ 1, SA, SB)                                                                               \
    {                                                                                                         \
      /* K-step instruction order pinned with sched_group_barrier (as in gconv_fast_kernel): the 16 LDS operand reads, */ \
      /* then the MFMA stream with the next tile's buffer loads dripped in, the LDS writes only after all but 6 MFMAs */ \
      /* -- without it the compiler hoists the writes (and the s_waitcnt on the loads just issued) to the top. */ \
      constexpr int NV = (AL4 ? A_V4 : 4 * A_V4) + RB, NM = 16 * TM * TN, PER = (NM - 10) / NV;               \
      __builtin_amdgcn_sched_group_barrier(0x100, 4 * (TM + TN), 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                      \
_Pragma("unroll")                                                                                             \
      for (int q_ = 0; q_ < NV; ++q_) {                                                                       \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                    \
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);                                                  \
      }                                                                                                       \
      __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 - PER * NV - 6, 0);                                  \
      __builtin_amdgcn_sched_group_barrier(0x200, A_V4 + RB, 0);                                              \
      __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);                                                      \
    }                                                                                                         \
    __syncthreads();                                                                                          \
  }
  {
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      HIM_WKSTEP(kt, raX, rbX, raY, rbY)
      HIM_WKSTEP(kt + 1, raY, rbY, raX, rbX)
    }
    if (kt < nk) HIM_WKSTEP(kt, raX, rbX, raY, rbY)
  }
#undef HIM_WKSTEP
#undef HIM_WM
#undef HIM_WLOAD
#undef HIM_WSTORE

  // tap-major slab: out[z][m][n']
  float* __restrict__ out = p.out + (size_t)blockIdx.z * p.M * p.Np;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int np = n0 + wn * TN * 32 + j * 32 + l31;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < p.M) out[(size_t)m * p.Np + np] = acc[i][j][r];
      }
    }
  }
}

// dW[m][ci][tap] (+)= sum_z slab[z][m][tap*C + ci]   (fixed summation order; coalesced on the dW side)
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                           int M, int C, int KK, int splits, int accumulate) {
  // one workgroup per (m, 64-channel chunk): slab rows [tap][64 ci] are read as 256-B runs (summed over the split-K
  // slabs in fixed order), transposed through LDS and written/accumulated as one contiguous [64 ci][KK] run
  __shared__ float sm[64 * 49];
  const int m = blockIdx.y, c0 = blockIdx.x * 64;
  const size_t n = (size_t)M * C * KK;
  const int nel = 64 * KK;
  for (int i = threadIdx.x; i < nel; i += 256) {
    const int tap = i >> 6, ci = i & 63;
    const size_t src = (size_t)m * C * KK + (size_t)tap * C + c0 + ci;
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += slabs[(size_t)z * n + src];
    sm[ci * KK + tap] = v;
  }
  __syncthreads();
  float* __restrict__ dst = dw + ((size_t)m * C + c0) * KK;
  for (int i = threadIdx.x; i < nel; i += 256) dst[i] = accumulate ? dst[i] + sm[i] : sm[i];
}

// the class (channels) of the fast family; its geometry part -- OH*OW >= 4 (planes with OH*OW % 4 != 0: scalar dY loads) and
// both tensors under 2 GiB (31-bit buffer offsets) -- is plan_wgrad's (him_conv.hip)
static bool wgrad_fast_class(const HimAlgo& a, int M, int C) { return !algo_off(a, HIM_ALGO_GENERIC_CONV) && M > 4 && (C % 64) == 0; }
static void wgrad_fast_cfg(const HimAlgo& a, int M, int C, int Kdim, int KK, int* BM, int* BN, int* splits) {
  // (64-row / 64-column tiles where 128 fit: no change of the step, round 3 -- unlike the conv kernel's tile)
  *BM = (M > 64 && a.wgrad_tile == 0) ? 128 : 64;
  *BN = ((C % 128) == 0 && a.wgrad_tile != 2) ? 128 : 64;
  const long long tiles = (long long)cdiv(M, *BM) * ((long long)C * KK / *BN);
  int s = (int)((768 + tiles - 1) / tiles);   // aim at 768 workgroups (384 / 1536: no change of the step, round 3)
  const int maxs = cdiv(Kdim, 32 * 8);
  if (s > maxs) s = maxs;
  if (s < 1) s = 1;
  if (s > 256) s = 256;
  if (a.wgrad_splits > 0) s = std::max(1, std::min(maxs, a.wgrad_splits));
  *splits = s;
}

// ---- tiny-M weight gradient (M = Cout <= 4: the G tanh head).  Direct VALU reduction: one workgroup per
// (input channel, slice of the B*OH*OW positions); every thread keeps the MM x TJ x TJ partial filter in
// registers, then a wave64-shuffle + LDS reduction writes one slab per slice (summed in fixed order later).
template <int MM, int TJ, bool REFLECT>
__global__ __launch_bounds__(256) void wgrad_small_kernel(const WGradP p) {
  __shared__ float red[4][MM * TJ * TJ];
  const int c = blockIdx.x;
  const int t = threadIdx.x;
  const int OHW = p.OH * p.OW, HW = p.H * p.W;
  const int kbeg = blockIdx.y * p.kchunk;
  const int kend = min(p.Kdim, kbeg + p.kchunk);
  float acc[MM][TJ][TJ];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int a = 0; a < TJ; ++a)
#pragma unroll
      for (int b2 = 0; b2 < TJ; ++b2) acc[m][a][b2] = 0.f;
  const int H = p.H, W = p.W;
  for (int k = kbeg + t; k < kend; k += 256) {
    const int b = k / OHW;
    const int sp = k - b * OHW;
    const int oh = (int)fdiv((uint32_t)sp, p.fOW);
    const int ow = sp - oh * p.OW;
    float g[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) g[m] = p.dy[((size_t)b * p.M + m) * OHW + sp];
    const float* __restrict__ xb = p.x + ((size_t)b * p.C + c) * HW;
    int ixs[TJ];
    bool okx[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      int ix = ow * p.stride - p.pad + j;
      bool ok = true;
      if (REFLECT) {
        ix = ix < 0 ? -ix : ix;
        ix = ix >= W ? 2 * (W - 1) - ix : ix;
      } else {
        const int cx = min(max(ix, 0), W - 1);
        ok = cx == ix;
        ix = cx;
      }
      ixs[j] = ix;
      okx[j] = ok;
    }
#pragma unroll
    for (int a = 0; a < TJ; ++a) {
      int iy = oh * p.stride - p.pad + a;
      bool oky = true;
      if (REFLECT) {
        iy = iy < 0 ? -iy : iy;
        iy = iy >= H ? 2 * (H - 1) - iy : iy;
      } else {
        const int cy = min(max(iy, 0), H - 1);
        oky = cy == iy;
        iy = cy;
      }
      const float* __restrict__ row = xb + (size_t)iy * W;
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        float v = row[ixs[j]];
        v = (oky && okx[j]) ? v : 0.f;
#pragma unroll
        for (int m = 0; m < MM; ++m) acc[m][a][j] = fmaf(g[m], v, acc[m][a][j]);
      }
    }
  }
  const int wave = t >> 6, lane = t & 63;
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int a = 0; a < TJ; ++a)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const float v = wave_sum(acc[m][a][j]);
        if (lane == 0) red[wave][(m * TJ + a) * TJ + j] = v;
      }
  __syncthreads();
  float* __restrict__ out = p.out + (size_t)blockIdx.y * p.M * p.Np;
  for (int i = t; i < MM * TJ * TJ; i += 256) {
    const int m = i / (TJ * TJ), r = i - m * TJ * TJ;
    out[(size_t)m * p.Np + c * TJ * TJ + r] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

__global__ void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, long long n,
                                   int splits, int accumulate) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slabs[(size_t)z * n + i];
    out[i] = accumulate ? out[i] + s : s;
  }
}

// dbias[c] (+)= sum_{b,sp} dy[b][c][sp]: stage 1 = (channel, slice) partial sums, stage 2 = fixed-order finish.
constexpr int BIAS_SLICES = 32;  // maximum; small planes use fewer (bias_slices())
static int bias_slices(int B, int hw) {
  long long per = ((long long)B * hw + 8191) / 8192;  // ~8k elements per workgroup
  if (per > BIAS_SLICES) per = BIAS_SLICES;
  if (per > hw) per = hw;
  return per < 1 ? 1 : (int)per;
}
// Bias gradients are sums of ~1e6 signed values that largely cancel (the head's: |sum| ~ 1e-2 of sum |dy|): fp32 partial
// sums left 1.6e-4 relative error against 2e-5 of torch's pairwise CPU sum (fp64-anchored step test).  The pass is
// HBM-bound and MI355X adds doubles at full vector rate, so every partial sum is carried in double.
__global__ __launch_bounds__(256) void bias_grad1_kernel(const float* __restrict__ dy, float* __restrict__ part,
                                                         int B, int C, int hw) {
  __shared__ double shd[4];
  const int c = blockIdx.x, sl = blockIdx.y;
  const int chunk = (hw + gridDim.y - 1) / gridDim.y;
  const int beg = sl * chunk, end = min(hw, beg + chunk);
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* pl = dy + ((size_t)b * C + c) * hw;
    for (int i = beg + threadIdx.x; i < end; i += 256) s += (double)pl[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = s;
  __syncthreads();
  // the slice sums travel as (hi, lo) float pairs: 48 significant bits through the fp32 workspace
  if (threadIdx.x == 0) {
    const double t = (shd[0] + shd[1]) + (shd[2] + shd[3]);
    const float hi = (float)t;
    part[(c * BIAS_SLICES + sl) * 2] = hi;
    part[(c * BIAS_SLICES + sl) * 2 + 1] = (float)(t - (double)hi);
  }
}
__global__ void bias_grad2_kernel(const float* __restrict__ part, float* __restrict__ db, int C, int nsl,
                                  int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int i = 0; i < nsl; ++i) s += (double)part[(c * BIAS_SLICES + i) * 2] + (double)part[(c * BIAS_SLICES + i) * 2 + 1];
  db[c] = accumulate ? db[c] + (float)s : (float)s;
}
static size_t bias_ws_bytes(int C) { return (size_t)C * BIAS_SLICES * 2 * sizeof(float) + 256; }

static int wgrad_splits(int M, int Np, int Kdim, int BM, int BN) {
  const long long tiles = (long long)cdiv(M, BM) * cdiv(Np, BN);
  int splits = (int)((1024 + tiles - 1) / tiles);
  const int maxs = cdiv(Kdim, 32 * 8);  // at least 8 K-steps per split
  if (splits > maxs) splits = maxs;
  if (splits < 1) splits = 1;
  if (splits > 512) splits = 512;
  return splits;
}
static void wgrad_tile(int M, int* BM, int* BN) {
  *BN = 128;
  *BM = M <= 32 ? 32 : (M <= 64 ? 64 : 128);
}


// sum over the 64 lanes of a wave with DPP row shifts + row broadcasts (full-rate VALU, no LDS crossbar); the total
// ends up in lane 63
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));  // row_shr:1
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));  // row_shr:2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));  // row_shr:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));  // row_shr:8
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, true));  // row_bcast:15
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, true));  // row_bcast:31
  return v;
}

// Tiny-M weight gradient for "same" odd kernels (the G tanh head conv7x7 64->3): sliding-window, lane-private.
// One wave = one input channel x one BAND of TR filter rows; its 64 lanes are 64 consecutive output columns and walk
// down a strip of rows keeping the TR x KS window of x around their pixel in registers (ONE new row of KS loads per step
// instead of KS*KS gathers), MM*TR*KS private FMA accumulators, a DPP wave reduction once per workgroup.
// The band split (blockIdx.z: filter rows [th0, th0+TR), th0 = min(z*TR, KS-TR); rows a later band recomputes are
// written by the later band only) keeps the 7x7 / 3-output case at ~160 VGPRs = 3 waves per SIMD -- the un-split
// kernel needed 278 registers, i.e. ONE wave per SIMD with nothing to hide its load latency behind.
// part[slot][m][c*KK + t].  grid (slots, ceil(C/4), ceil(KS/TR)); workgroups are persistent over the (image, column
// strip, row chunk) tasks.
template <int MM, int KS, int TR, bool REFLECT>
__global__ __launch_bounds__(256) void wgrad_small_win_kernel(const WGradP p, int nsx, int nyc, int rows_per, int ntasks) {
  constexpr int KK = KS * KS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.y * 4 + wave;
  if (c >= p.C) return;
  const int th0 = min((int)blockIdx.z * TR, KS - TR);      // first filter row of this band
  const int own0 = (int)blockIdx.z * TR - th0;             // band rows [own0, TR) are written by this band
  const int H = p.H, W = p.W, HW = H * W, pad = p.pad;
  const int padr = pad - th0;                              // row padding as seen by the band
  float acc[MM][TR * KS];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int t = 0; t < TR * KS; ++t) acc[m][t] = 0.f;
  for (int task = blockIdx.x; task < ntasks; task += gridDim.x) {
    int q = task;
    const int yc = q % nyc;
    q /= nyc;
    const int sx = q % nsx, b = q / nsx;
    const int px = sx * 64 + lane;
    const bool lane_on = px < W;
    const int y0 = yc * rows_per, y1 = min(y0 + rows_per, H);
    const float* __restrict__ xc = p.x + ((size_t)b * p.C + c) * HW;
    const float* __restrict__ g = p.dy + (size_t)b * p.M * HW + min(px, W - 1);
    int cx[KS];
    bool okc[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      int ix = px - pad + k;
      bool ok = lane_on;
      if (REFLECT) {
        ix = ix < 0 ? -ix : ix;
        ix = ix >= W ? 2 * (W - 1) - ix : ix;
      } else {
        ok = ok && ix >= 0 && ix < W;
      }
      cx[k] = min(max(ix, 0), W - 1);
      okc[k] = ok;
    }
    float win[TR][KS];
#define HIM_SW_ROW(PY, DST)                                                            \
  {                                                                                    \
    int iy = (PY);                                                                     \
    bool oky = true;                                                                   \
    if (REFLECT) {                                                                     \
      iy = iy < 0 ? -iy : iy;                                                          \
      iy = iy >= H ? 2 * (H - 1) - iy : iy;                                            \
    } else {                                                                           \
      oky = iy >= 0 && iy < H;                                                         \
    }                                                                                  \
    const float* __restrict__ rp = xc + min(max(iy, 0), H - 1) * W;                    \
    _Pragma("unroll") for (int k = 0; k < KS; ++k) {                                   \
      const float v = rp[cx[k]];                                                       \
      DST[k] = (oky && okc[k]) ? v : 0.f;                                              \
    }                                                                                  \
  }
#pragma unroll
    for (int r = 0; r < TR; ++r) HIM_SW_ROW(y0 - padr + r, win[r])
    float gv[MM], gn[MM];   // dy of this row / of the next one (loaded a step ahead)
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      const float v = g[(size_t)m * HW + y0 * W];
      gn[m] = lane_on ? v : 0.f;
    }
    float nxt[KS], nx2[KS];   // x rows entering the window one / two steps from now
    HIM_SW_ROW(y0 - padr + TR, nxt)
    for (int pyb = y0; pyb < y1; pyb += TR) {
#pragma unroll
      for (int ph = 0; ph < TR; ++ph) {
        const int py = pyb + ph;
        if (py < y1) {
          HIM_SW_ROW(py - padr + TR + 1, nx2)
#pragma unroll
          for (int m = 0; m < MM; ++m) {
            gv[m] = gn[m];
            const float v = g[(size_t)m * HW + min(py + 1, H - 1) * W];
            gn[m] = lane_on ? v : 0.f;
          }
          // x row (py - padr + th) sits in logical slot th = physical (th + ph) % TR
#pragma unroll
          for (int th = 0; th < TR; ++th)
#pragma unroll
            for (int tw = 0; tw < KS; ++tw)
#pragma unroll
              for (int m = 0; m < MM; ++m) acc[m][th * KS + tw] = fmaf(gv[m], win[(th + ph) % TR][tw], acc[m][th * KS + tw]);
#pragma unroll
          for (int k = 0; k < KS; ++k) {
            win[ph][k] = nxt[k];
            nxt[k] = nx2[k];
          }
        }
      }
    }
#undef HIM_SW_ROW
  }
  float* __restrict__ out = p.out + (size_t)blockIdx.x * p.M * p.Np + (size_t)c * KK;
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int th = 0; th < TR; ++th)
#pragma unroll
      for (int tw = 0; tw < KS; ++tw) {
        const float sm = wave_sum_dpp(acc[m][th * KS + tw]);
        if (lane == 63 && th >= own0) out[(size_t)m * p.Np + (th0 + th) * KS + tw] = sm;
      }
}

