// -*- c++ -*-
// =============================================================================================
// Weight gradient of "same" odd-kernel stride-1 convolutions with <= 4 channels on ONE side, on the matrix cores:
//   HEAD  (Cout <= 4: the generators' tanh head conv7x7 64 -> 3):  dW[m][c][kh][kw] = sum dy[m][y][x] * xpad[c][y+kh][x+kw]
//   STEM  (Cin  <= 4: the dense image channels of the first conv 3 -> 64): same sum, the roles of the tensors swapped.
// Both are dense contractions over the pixels with a 64-wide side (T, the "wide" tensor) and a <= 4-wide side (S).  The
// direct VALU form (wgrad_small_win_kernel) reached 10 TFLOP/s: 147 accumulators per lane, every x value loaded 7 times.
// Here the contraction index k runs over the COLUMNS of one row of T, the matrix rows are T's channels, and the matrix
// columns n = (s, kw) pair a narrow channel with a horizontal tap: B[k][n] = S[s][k -/+ kw] is a Toeplitz operand read
// straight from an LDS copy of S's row (21 of 32 columns live for 3 channels x 7 taps).  The 7 vertical taps are 7
// accumulator sets fed by the SAME A operand (T's row) and 7 different rows of S held in an LDS ring, so T -- 95 % of
// the bytes -- is read exactly once:  per 2 columns of a row 2 + 7 ds_read_b32 feed 14 v_mfma_f32_32x32x2f32.
//   executed 2*64*32*49 FLOP per pixel (N padded 21 -> 32), 262 x 518 padded pixels x 8 images: 0.23 ms of matrix-pipe
//   time at C2 against 1.86 ms of the VALU kernel; HBM: T once (268 MB), S seven times (12.6 MB each).
// One workgroup = 4 waves = one (image, 128-column chunk, row band) task at a time (persistent over the tasks); wave w
// owns columns [32w, 32w+32) of the chunk and ALL 7 x 2 accumulator tiles (224 registers, one wave per SIMD).  The next
// row of T travels global -> registers before the MFMA block and registers -> LDS after it (two LDS buffers).
// The waves of a workgroup add their partial tiles in LDS in wave order; wgrad_fewch_finish_kernel adds the workgroups'
// partials in slot order.
// =============================================================================================
struct FewChP {
  const float* T;   // wide tensor   [B][TC][H][W]
  const float* S;   // narrow tensor [B][SC][H][W]
  float* part;      // [workgroups][KS][CT][16][64]
  int B, TC, SC, H, W, pad, reflect;
  int head;         // 1: T = x (walked in PADDED coordinates), S = dy;  0: T = dy, S = x (padded coordinates)
  int TH, TW;       // extent of the walk over T: head (H + 2 pad, W + 2 pad), stem (H, W)
  int nchunk, nband, rows_per, ntask;
};

static __device__ __forceinline__ int fewch_map(int i, int n, bool reflect) {   // padded -> source index, -1 = zero
  if (reflect) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i;
  }
  return (i < 0 || i >= n) ? -1 : i;
}

template <int KS, int CT>
__global__ __launch_bounds__(256) void wgrad_fewch_mfma_kernel(const FewChP p) {
  typedef float f16v __attribute__((ext_vector_type(16)));
  constexpr int QC = 128, QS = QC + 1;          // chunk columns; odd LDS row stride (lanes of an A read walk the channels)
  constexpr int SWS = QC + 8;                   // S row: chunk + KS-1 halo columns
  constexpr int RING = 8;                       // 7 live S rows + the one being filled
  __shared__ float Ts[2][CT * 32][QS];
  __shared__ float Ss[RING + 1][4][SWS];        // slot RING stays zero (dead matrix columns read it)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int H = p.H, W = p.W, pad = p.pad;
  const bool refl = p.reflect != 0, head = p.head != 0;
  const int cgrp = blockIdx.y * CT * 32;        // first wide channel of this workgroup
  f16v acc[KS][CT];
#pragma unroll
  for (int a = 0; a < KS; ++a)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
  for (int i = tid; i < 4 * SWS; i += 256) (&Ss[RING][0][0])[i] = 0.f;
  // matrix column of this lane: n = l31 = s * 8 + kw
  const int ns = l31 >> 3, nkw = l31 & 7;
  const bool ncol_live = ns < p.SC && nkw < KS;
  const int boff_lane = head ? (KS - 1 - nkw) : nkw;          // j = ql - kw + (KS-1)   |   j = ql + kw
  constexpr int TPT = CT * 32 * QC / 256;                     // T elements per thread and row (16 or 32)
  const int tq = tid & (QC - 1), tc0 = tid >> 7;              // this thread's column in the chunk / first channel (step 2)

  for (int task = blockIdx.x; task < p.ntask; task += gridDim.x) {
    int q = task;
    const int chunk = q % p.nchunk;
    q /= p.nchunk;
    const int band = q % p.nband, b = q / p.nband;
    const int q0 = chunk * QC;                                 // first T column of the chunk
    const int r0 = band * p.rows_per, r1 = min(r0 + p.rows_per, p.TH);
    const int ncol = min(QC, p.TW - q0);                       // valid T columns in the chunk
    const float* __restrict__ Tb = p.T + ((size_t)b * p.TC + cgrp) * H * W;
    const float* __restrict__ Sb = p.S + (size_t)b * p.SC * H * W;
    // source column of this thread's T element (head: padded -> x column), -1 = zero
    int tcol = -1;
    if (tq < ncol) tcol = head ? fewch_map(q0 + tq - pad, W, refl) : (q0 + tq);
    float treg[TPT];
    // ---- helpers -------------------------------------------------------------------------------------------------
    auto load_T = [&](int r) {                                 // row r of the walk -> registers
      const int srow = head ? fewch_map(r - pad, H, refl) : r;
      const bool ok = srow >= 0 && tcol >= 0 && r < r1;
      const float* __restrict__ src = Tb + (size_t)max(srow, 0) * W + max(tcol, 0);
#pragma unroll
      for (int i = 0; i < TPT; ++i) {
        const float v = ok ? src[(size_t)(tc0 + 2 * i) * H * W] : 0.f;
        treg[i] = v;
      }
    };
    auto store_T = [&](int buf) {
#pragma unroll
      for (int i = 0; i < TPT; ++i) Ts[buf][tc0 + 2 * i][tq] = treg[i];
    };
    auto fill_S = [&](int sigma) {                             // S row sigma -> ring slot (sigma & 7)
      // head: sigma = dy row (zero outside [0,H)), local column j <-> dy column q0 + j - (KS-1)
      // stem: sigma = PADDED x row,                local column j <-> padded x column q0 + j
      const int slot = (sigma + 64) & (RING - 1);
      const int srow = head ? ((sigma >= 0 && sigma < H) ? sigma : -1) : fewch_map(sigma - pad, H, refl);
      for (int e = tid; e < p.SC * SWS; e += 256) {
        const int s = e / SWS, j = e - s * SWS;
        const int scol = head ? (q0 + j - (KS - 1)) : fewch_map(q0 + j - pad, W, refl);
        const bool ok = srow >= 0 && scol >= 0 && scol < W;
        Ss[slot][s][j] = ok ? Sb[((size_t)s * H + srow) * W + scol] : 0.f;
      }
    };
    // ---- prologue: the S rows the first T row meets, the first T row ----------------------------------------------
    __syncthreads();                                           // previous task's readers are done
    if (head) {
      for (int a = 0; a < KS; ++a) fill_S(r0 - a);             // dy rows r0 - kh
    } else {
      for (int a = 0; a < KS; ++a) fill_S(r0 + a);             // padded x rows r0 + kh
    }
    load_T(r0);
    store_T(0);
    __syncthreads();
    int buf = 0;
    const int ksteps = max(0, min(16, (ncol - wave * 32 + 1) >> 1));   // live 2-column steps of this wave
    for (int r = r0; r < r1; ++r) {
      if (r + 1 < r1) load_T(r + 1);                           // global -> registers, in flight across the MFMA block
      // ---- 7 x CT accumulator tiles over this wave's 32 columns -------------------------------------------------
      const float* __restrict__ ta = &Ts[buf][l31][wave * 32 + lh];
      const float* sb[KS];
#pragma unroll
      for (int a = 0; a < KS; ++a) {
        const int sigma = head ? (r - a) : (r + a);
        const int slot = ncol_live ? ((sigma + 64) & (RING - 1)) : RING;
        sb[a] = &Ss[slot][ncol_live ? ns : 0][wave * 32 + lh + boff_lane];
      }
      for (int ks = 0; ks < ksteps; ++ks) {
        float av[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) av[c] = ta[c * 32 * QS + 2 * ks];
#pragma unroll
        for (int a = 0; a < KS; ++a) {
          const float bv = sb[a][2 * ks];
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bv, acc[a][c], 0, 0, 0);
        }
      }
      if (r + 1 < r1) {
        store_T(buf ^ 1);
        fill_S(head ? (r + 1) : (r + KS));                     // the one new S row of the next step
      }
      __syncthreads();
      buf ^= 1;
    }
  }
  // ---- the four waves add their 7 x CT tiles in LDS in wave order (fixed summation order), then the workgroup writes
  // ONE partial: part[wg][kh][ct][reg][lane]  (round 3b: per-wave partials were 58.7 MB per launch and a 0.12 ms finish)
  float* __restrict__ red = &Ts[0][0][0];
  static_assert(2 * CT * 32 * QS >= KS * CT * 1024, "tile partials must fit the T buffers");
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < KS; ++a)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int idx = ((a * CT + c) * 16 + r) * 64 + lane;
            red[idx] = (w == 0 ? 0.f : red[idx]) + acc[a][c][r];
          }
    }
  }
  __syncthreads();
  const int slot = (int)blockIdx.y * gridDim.x + blockIdx.x;
  float* __restrict__ out = p.part + (size_t)slot * KS * CT * 1024;
  for (int i = tid; i < KS * CT * 1024; i += 256) out[i] = red[i];
}

// dW (+)= sum over the wave slots, in slot order.  grid (KS * CT * 16, TC / (32 CT)), 256 threads: wave w sums slots
// w, w+4, ...; lanes = the 64 (row half, column) positions of accumulator register `reg`.
template <int KS, int CT>
__global__ __launch_bounds__(256) void wgrad_fewch_finish_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                int nslot_per_grp, int head, int M, int C, int SC,
                                                                int accumulate) {
  __shared__ float sh[4][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x;                       // (kh, ct, reg)
  const int reg = item & 15, ct = (item >> 4) % CT, kh = item / (16 * CT);
  const float* __restrict__ src = part + (size_t)blockIdx.y * nslot_per_grp * KS * CT * 1024 + (size_t)item * 64 + lane;
  float s = 0.f;
  for (int sl = wave; sl < nslot_per_grp; sl += 4) s += src[(size_t)sl * KS * CT * 1024];
  sh[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  s = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
  const int l31 = lane & 31, lh = lane >> 5;
  const int tch = blockIdx.y * CT * 32 + ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;   // wide channel
  const int sc = l31 >> 3, kw = l31 & 7;
  if (sc >= SC || kw >= KS) return;
  const int m = head ? sc : tch, c = head ? tch : sc;
  float* __restrict__ o = dw + (((size_t)m * C + c) * KS + kh) * KS + kw;
  *o = accumulate ? *o + s : s;
}

static const int FEWCH_WGS = 256;
static bool fewch_off(const HimAlgo& a) { return algo_off(a, HIM_ALGO_NO_FEWCH_MFMA); }
// The class (channels and kernel) of the few-channel families: `narrow` <= 4 channels on one side, `wide` % 32 == 0 on the
// other.  head: (M, C) = (narrow, wide); stem: (C, M).  The geometry part is wgrad_same_geom (him_conv.hip plan_wgrad).
static bool fewch_class(const HimAlgo& a, int narrow, int wide, int KH, int KW) {
  return !fewch_off(a) && narrow <= 4 && wide >= 32 && (wide % 32) == 0 && KH == KW && (KH == 5 || KH == 7);
}
static int fewch_groups(int TC, int* CT) {
  *CT = (TC % 64) == 0 ? 2 : 1;
  return TC / (32 * *CT);
}
// bytes of the `wgs` workgroups' partial tiles
static size_t fewch_need_bytes(int TC, int KS, int wgs) {
  int CT;
  const int grp = fewch_groups(TC, &CT);
  return (size_t)grp * wgs * KS * CT * 1024 * sizeof(float);
}
// the walk over the wide tensor: chunks of 128 columns x row bands x images = tasks
static FewChP fewch_geom(bool head, int B, int H, int W, int pad) {
  FewChP p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.H = H; p.W = W; p.pad = pad;
  p.head = head ? 1 : 0;
  p.TH = head ? H + 2 * pad : H;
  p.TW = head ? W + 2 * pad : W;
  p.nchunk = cdiv(p.TW, 128);
  // row bands: enough tasks to give every workgroup a few (the S-ring warm-up costs KS-1 extra rows per band)
  int nband = std::max(1, (4 * FEWCH_WGS) / std::max(1, B * p.nchunk));
  nband = std::min(nband, std::max(1, p.TH / 16));
  p.rows_per = cdiv(p.TH, nband);
  p.nband = cdiv(p.TH, p.rows_per);
  p.ntask = B * p.nchunk * p.nband;
  return p;
}
// wgs = min(tasks, FEWCH_WGS) workgroups (the plan's `splits`); ws holds fewch_need_bytes(TC, KS, wgs)
static int run_wgrad_fewch(bool head, const float* dy, const float* x, float* dw, int M, int C, int B, int H, int W, int KS,
                           int pad, int pad_mode, int wgs, int accumulate, void* ws, hipStream_t st) {
  FewChP p = fewch_geom(head, B, H, W, pad);
  p.T = head ? x : dy;
  p.S = head ? dy : x;
  p.TC = head ? C : M;
  p.SC = head ? M : C;
  p.reflect = pad_mode == HIM_PAD_REFLECT ? 1 : 0;
  int CT;
  const int grp = fewch_groups(p.TC, &CT);
  p.part = (float*)ws;
  const dim3 grid(wgs, grp), block(256);
#define HIM_FEWCH(KSv, CTv)                                                                                              \
  if (KS == KSv && CT == CTv) {                                                                                          \
    hipLaunchKernelGGL((wgrad_fewch_mfma_kernel<KSv, CTv>), grid, block, 0, st, p);                                      \
    hipLaunchKernelGGL((wgrad_fewch_finish_kernel<KSv, CTv>), dim3(KSv * CTv * 16, grp), block, 0, st,                   \
                       (const float*)ws, dw, wgs, p.head, M, C, p.SC, accumulate);                                   \
  }
  HIM_FEWCH(5, 1) HIM_FEWCH(5, 2) HIM_FEWCH(7, 1) HIM_FEWCH(7, 2)
#undef HIM_FEWCH
  return check_launch("wgrad_fewch_mfma");
}
