// -*- c++ -*-
// =============================================================================================
// ResnetBlock  out = x + IN(conv3x3(refpad(ReLU(IN(conv3x3(refpad(x)))))))   (reference models/layer_util.py:333-378)
// on the separate-transform Winograd pipeline with both InstanceNorms folded into the transforms
// (north star: "fused Conv2d+InstanceNorm" blocks; reference get_norm_layer, models/layer_util.py:19-26):
//   * statistics in the OUTPUT transform: one workgroup owns a whole (image, channel) plane -- at the ResnetBlock stack
//     a plane is 16x32 pixels = 128 tiles -- so it can reduce mean / variance while it un-transforms (wino_out_stats);
//   * normalisation + ReLU ON LOAD in the next convolution's input transform (wino_input_kernel<.., NORM>): the
//     normalised activation is never written or re-read; the weight-gradient transform recomputes it the same way;
//   * the block tail applies IN + residual in the output transform that produced the statistics;
//   * backward: the data gradient's output transform applies the ReLU gate and the InstanceNorm backward of the plane
//     it has just produced (wino_out_inbwd); the skip-path gradient is added by the last output transform.
// Against the unfused layer sequence a block saves 3 launches forward / 2 backward and ~170 MB of plane round trips.
// Saved for backward: x, the raw conv outputs y1 / y2 and their per-plane [mean | rstd].
// =============================================================================================

// y[b][c] = A^T Mo A + bias (raw conv output, kept for backward); stat = [mean | rstd]; RES: out = (y - mean) rstd + res.
// grid (B*C), one plane per workgroup; plane <= 4096 pixels.
template <bool RES>
__global__ __launch_bounds__(256) void wino_out_stats_kernel(const float* __restrict__ Mo, const float* __restrict__ bias,
                                                             const float* __restrict__ res, float* __restrict__ y,
                                                             float* __restrict__ stat, float* __restrict__ out,
                                                             const WinoGeom g, float eps) {
  __shared__ float pl[4096];
  __shared__ float sh[8];
  const int plane = blockIdx.x, b = plane / g.C, c = plane - b * g.C, tid = threadIdx.x;
  const int per = g.TY * g.TX, hw = g.OH * g.OW;
  const size_t slab = (size_t)g.C * g.Tp;
  const float bb = bias ? bias[c] : 0.f;
  float s = 0.f;
  for (int tl = tid; tl < per; tl += 256) {
    const float* __restrict__ in = Mo + (size_t)c * g.Tp + (size_t)b * per + tl;
    float m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) m[i][j] = in[(size_t)(i * 4 + j) * slab];
    float r[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[0][j] = m[0][j] + m[1][j] + m[2][j];
      r[1][j] = m[1][j] - m[2][j] - m[3][j];
    }
    const int ty = tl / g.TX, tx = tl - ty * g.TX;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float v0 = r[i][0] + r[i][1] + r[i][2] + bb, v1 = r[i][1] - r[i][2] - r[i][3] + bb;
      pl[(2 * ty + i) * g.OW + 2 * tx] = v0;
      pl[(2 * ty + i) * g.OW + 2 * tx + 1] = v1;
      s += v0 + v1;
    }
  }
  const float mu = block_sum_256(s, sh) / (float)hw;       // (the barriers inside also publish pl[])
  float q = 0.f;
  for (int i = tid; i < hw; i += 256) {
    const float d = pl[i] - mu;
    q += d * d;
  }
  const float var = block_sum_256(q, sh) / (float)hw;       // biased variance, centred second pass (as instnorm_fwd)
  const float rs = 1.f / sqrtf(var + eps);
  if (tid == 0) {
    stat[plane] = mu;
    stat[g.B * g.C + plane] = rs;
  }
  float* __restrict__ yp = y + (size_t)plane * hw;
  for (int i = tid; i < hw; i += 256) yp[i] = pl[i];
  if (RES) {
    const float* __restrict__ rp = res + (size_t)plane * hw;
    float* __restrict__ op = out + (size_t)plane * hw;
    for (int i = tid; i < hw; i += 256) op[i] = (pl[i] - mu) * rs + rp[i];
  }
}

// dy[b][c] = InstanceNorm backward of dz = (A^T Md A) * [xhat > 0],  xhat = (y - mean) rstd   (ReLU behind the norm):
//   dy = rstd * (dz - mean(dz) - xhat * mean(dz * xhat)).   grid (B*C)
__global__ __launch_bounds__(256) void wino_out_inbwd_kernel(const float* __restrict__ Md, const float* __restrict__ y,
                                                             const float* __restrict__ stat, float* __restrict__ dy,
                                                             const WinoGeom g) {
  __shared__ float pl[4096];
  __shared__ float sh[8];
  const int plane = blockIdx.x, b = plane / g.C, c = plane - b * g.C, tid = threadIdx.x;
  const int per = g.TY * g.TX, hw = g.OH * g.OW;
  const size_t slab = (size_t)g.C * g.Tp;
  for (int tl = tid; tl < per; tl += 256) {
    const float* __restrict__ in = Md + (size_t)c * g.Tp + (size_t)b * per + tl;
    float m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) m[i][j] = in[(size_t)(i * 4 + j) * slab];
    float r[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r[0][j] = m[0][j] + m[1][j] + m[2][j];
      r[1][j] = m[1][j] - m[2][j] - m[3][j];
    }
    const int ty = tl / g.TX, tx = tl - ty * g.TX;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      pl[(2 * ty + i) * g.OW + 2 * tx] = r[i][0] + r[i][1] + r[i][2];
      pl[(2 * ty + i) * g.OW + 2 * tx + 1] = r[i][1] - r[i][2] - r[i][3];
    }
  }
  __syncthreads();
  const float mu = stat[plane], rs = stat[g.B * g.C + plane];
  const float* __restrict__ yp = y + (size_t)plane * hw;
  float s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < hw; i += 256) {
    const float xh = (yp[i] - mu) * rs;
    const float dz = xh > 0.f ? pl[i] : 0.f;
    pl[i] = dz;                        // each element is owned by one thread
    s1 += dz;
    s2 += dz * xh;
  }
  const float m1 = block_sum_256(s1, sh) / (float)hw;
  const float m2 = block_sum_256(s2, sh) / (float)hw;
  float* __restrict__ op = dy + (size_t)plane * hw;
  for (int i = tid; i < hw; i += 256) {
    const float xh = (yp[i] - mu) * rs;
    op[i] = rs * (pl[i] - m1 - xh * m2);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
static HimConv2d resblock_conv_desc(const HimResBlock* d) {
  HimConv2d c;
  memset(&c, 0, sizeof(c));
  c.B = d->B; c.Cin = d->C; c.Cout = d->C; c.H = d->H; c.W = d->W; c.OH = d->H; c.OW = d->W;
  c.KH = c.KW = 3; c.stride = 1; c.pad = 1; c.pad_mode = HIM_PAD_REFLECT; c.act = HIM_ACT_NONE;
  c.algo = d->algo;
  c.algo.disable &= ~HIM_ALGO_WINO4_TRAIN_FWD;   // the block runs its own F(2x2) pipeline whatever the layerwise forward would take
  return c;
}
static bool resblock_ok(const HimResBlock* d) {
  if (!d || algo_off(d->algo, HIM_ALGO_NO_RESBLOCK_FUSED) || d->B <= 0 || d->C <= 0 || d->H < 4 || d->W < 4) return false;
  const HimConv2d c = resblock_conv_desc(d);
  if (check_conv(&c)) return false;
  // the separate-transform Winograd pipeline in all three directions (the fused single-launch kernel owns <= 512 channels),
  // the reflect gradient folded into the border patches (even planes), a plane that fits one workgroup's LDS
  const ConvPlan g = plan_dgrad(&c, false);
  return plan_fprop(&c).family == CONV_WINO && g.family == CONV_WINO && g.wino_fold &&
         wino_wgrad_ok(d->algo, d->C, d->C, 3, 3, 1, 1, d->H, d->W) && d->H * d->W <= 4096;
}
static size_t resblock_ws_floats(const HimResBlock* d) {   // V + M of one convolution
  const WinoGeom g = wino_geom(d->B, d->C, d->H, d->W, d->H, d->W, 1);
  return (size_t)2 * 16 * d->C * g.Tp;
}

extern "C" {

int him_resblock_supported(const HimResBlock* d) { return resblock_ok(d) ? 1 : 0; }
size_t him_resblock_ws(const HimResBlock* d) { return resblock_ok(d) ? resblock_ws_floats(d) * sizeof(float) + 256 : 0; }
size_t him_resblock_bwd_weight_ws(const HimResBlock* d) {
  return resblock_ok(d) ? wino_wgrad_floats(d->B, d->C, d->C, d->H, d->W) * sizeof(float) + 256 : 0;
}

int him_resblock_fwd(const HimResBlock* d, const float* x, const void* panel1, const float* bias1, const void* panel2,
                     const float* bias2, float* y1, float* stat1, float* y2, float* stat2, float* out, void* ws,
                     size_t ws_bytes, void* stream) {
  if (!resblock_ok(d)) return fail(HIM_E_UNSUPPORTED, "resblock: unsupported shape");
  if (!ws || ws_bytes < him_resblock_ws(d)) return fail(HIM_E_WORKSPACE, "resblock fwd: ws too small");
  hipStream_t st = (hipStream_t)stream;
  const WinoGeom g = wino_geom(d->B, d->C, d->H, d->W, d->H, d->W, 1);
  float* V = (float*)ws;
  float* Mo = V + (size_t)16 * d->C * g.Tp;
  const dim3 gin(cdiv(g.Tp, 256), d->C), blk(256);
  hipLaunchKernelGGL((wino_input_kernel<true, false>), gin, blk, 0, st, x, V, g, (const float*)nullptr);
  int rc = wino_batched_gemm(d->algo, (const float*)panel1, V, Mo, d->C, d->C, g.Tp, st);
  if (rc) return rc;
  hipLaunchKernelGGL((wino_out_stats_kernel<false>), dim3(d->B * d->C), blk, 0, st, (const float*)Mo, bias1,
                     (const float*)nullptr, y1, stat1, (float*)nullptr, g, d->eps);
  hipLaunchKernelGGL((wino_input_kernel<true, true>), gin, blk, 0, st, (const float*)y1, V, g, (const float*)stat1);
  rc = wino_batched_gemm(d->algo, (const float*)panel2, V, Mo, d->C, d->C, g.Tp, st);
  if (rc) return rc;
  hipLaunchKernelGGL((wino_out_stats_kernel<true>), dim3(d->B * d->C), blk, 0, st, (const float*)Mo, bias2, x, y2, stat2,
                     out, g, d->eps);
  return check_launch("resblock_fwd");
}

/* g = dL/d(out).  Writes dy2 = dL/d(y2), dy1 = dL/d(y1) (both needed by him_resblock_bwd_weight) and dx = dL/d(x)
 * (conv path + the skip path's g).  panel*_bwd: HIM_PANEL_BWD_DATA panels of the two convolutions. */
int him_resblock_bwd_data(const HimResBlock* d, const float* g_out, const float* y1, const float* stat1, const float* y2,
                          const float* stat2, const void* panel1_bwd, const void* panel2_bwd, float* dy2, float* dy1,
                          float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (!resblock_ok(d)) return fail(HIM_E_UNSUPPORTED, "resblock: unsupported shape");
  if (!ws || ws_bytes < him_resblock_ws(d)) return fail(HIM_E_WORKSPACE, "resblock bwd: ws too small");
  hipStream_t st = (hipStream_t)stream;
  WinoGeom g = wino_geom(d->B, d->C, d->H, d->W, d->H, d->W, 1);
  float* V = (float*)ws;
  float* Mo = V + (size_t)16 * d->C * g.Tp;
  const dim3 gin(cdiv(g.Tp, 256), d->C), blk(256);
  // tail norm (no activation behind it): dy2 = INbwd(g)
  int rc = him_instnorm_bwd(y2, stat2, stat2 + (size_t)d->B * d->C, g_out, dy2, d->B * d->C, d->H * d->W, HIM_ACT_NONE, 0.f,
                            stream);
  if (rc) return rc;
  WinoGeom gf = g;
  gf.fold = 1;      // reflect-pad data gradient folded into the border tiles' patches
  hipLaunchKernelGGL((wino_input_kernel<false, false>), gin, blk, 0, st, (const float*)dy2, V, gf, (const float*)nullptr);
  rc = wino_batched_gemm(d->algo, (const float*)panel2_bwd, V, Mo, d->C, d->C, g.Tp, st, true);
  if (rc) return rc;
  hipLaunchKernelGGL(wino_out_inbwd_kernel, dim3(d->B * d->C), blk, 0, st, (const float*)Mo, y1, stat1, dy1, g);
  hipLaunchKernelGGL((wino_input_kernel<false, false>), gin, blk, 0, st, (const float*)dy1, V, gf, (const float*)nullptr);
  rc = wino_batched_gemm(d->algo, (const float*)panel1_bwd, V, Mo, d->C, d->C, g.Tp, st, true);
  if (rc) return rc;
  hipLaunchKernelGGL(wino_output_kernel, dim3(cdiv(g.Tp, 256), d->C), blk, 0, st, (const float*)Mo, dx,
                     (const float*)nullptr, g, (int)HIM_ACT_NONE, 0.f, g_out);
  return check_launch("resblock_bwd_data");
}

/* dw (+)= weight gradient of convolution `which` (1: input x; 2: input relu(IN(y1)), recomputed on load from y1 / stat1) */
int him_resblock_bwd_weight(const HimResBlock* d, int which, const float* src, const float* stat, const float* dy, float* dw,
                            int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (!resblock_ok(d)) return fail(HIM_E_UNSUPPORTED, "resblock: unsupported shape");
  if (which != 1 && which != 2) return fail(HIM_E_INVALID, "resblock: which must be 1 or 2");
  if (!ws || ws_bytes < him_resblock_bwd_weight_ws(d)) return fail(HIM_E_WORKSPACE, "resblock wgrad: ws too small");
  hipStream_t st = (hipStream_t)stream;
  const WinoGeom g = wino_geom(d->B, d->C, d->H, d->W, d->H, d->W, 1);
  float* Vt = (float*)ws;                            // [16][Tp][C]
  float* dM = Vt + (size_t)16 * d->C * g.Tp;         // [16][C][Tp]
  float* dU = dM + (size_t)16 * d->C * g.Tp;         // [16][C][C]
  const dim3 gin(cdiv(d->C, 256), g.Tp), blk(256);
  if (which == 2) hipLaunchKernelGGL((wino_input_t_kernel<true, true>), gin, blk, 0, st, src, Vt, g, stat);
  else hipLaunchKernelGGL((wino_input_t_kernel<true, false>), gin, blk, 0, st, src, Vt, g, (const float*)nullptr);
  hipLaunchKernelGGL(wino_dy_kernel, dim3(cdiv(g.Tp, 256), d->C), blk, 0, st, dy, dM, g);
  int rc = wino_batched_gemm(d->algo, dM, Vt, dU, d->C, g.Tp, d->C, st);
  if (rc) return rc;
  hipLaunchKernelGGL(wino_wgrad_out_kernel, dim3(cdiv(d->C, 256), d->C), blk, 0, st, (const float*)dU, dw, d->C, d->C,
                     accumulate);
  return check_launch("resblock_bwd_weight");
}

}  // extern "C"
