// The fp64 matrix-core Gram tile shared by him_featdist.hip (KID) and him_prdc.hip (k-NN): the dot products of 32 rows
// of one fp32 matrix with 32 rows of another on v_mfma_f64_16x16x4_f64, operands widened on load.  A product of two fp32
// values is exact in fp64, so only the summation rounds, and its order is fixed by the K loop below.
//
// Fragment layout of v_mfma_f64_16x16x4_f64 (one f64 per lane for A and B, four per lane for C/D):
//   A[m][k]: m = lane & 15, k = lane >> 4        B[k][n]: k = lane >> 4, n = lane & 15
//   C/D register q: column n = lane & 15, row m = (lane >> 4) + 4 q      (NOT the f32 map 4 (lane >> 4) + q)
#pragma once
#include "him_common.h"

namespace him {

typedef double mfma_d4 __attribute__((ext_vector_type(4)));

// o[j] = row[k + j] widened, zero from column D on.  vec (gram_vec_ok): one 16-byte load; k + 3 < D follows from k < D.
__device__ __forceinline__ void gram_load4(const float* __restrict__ row, int k, int D, bool vec, double* o) {
  if (vec && k < D) {
    const float4 v = *(const float4*)(row + k);
    o[0] = (double)v.x, o[1] = (double)v.y, o[2] = (double)v.z, o[3] = (double)v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = k + j < D ? (double)row[k + j] : 0.0;
  }
}

// A wave's 32 x 32 block as 2 x 2 accumulators: acc[u][v] = the 16 x 16 products of the A rows pa<u> with the B rows
// pb<v>, where pa<u> / pb<v> is the row (of D columns) this lane's m = n = lane & 15 stands for in block u / v, and
// g = lane >> 4 is the lane's k group.  The caller resolves the rows -- every pointer must be readable for D floats --
// and masks what lies outside its matrix.  A lane loads four consecutive columns of its rows and feeds them to four
// instructions: instruction j multiplies the columns k0 + 4 g' + j, g' = 0..3.  Both operands permute k the same way,
// so every instruction still multiplies matching columns.
// The shape of the interface is measured, not taste: row pointers by value, `vec` as the kernels' int argument and
// tested at the load, g from the caller.  With that kid_tile_kernel runs at the speed of its former private loop; with
// array references, a bool and lane >> 4 inside, the same loop got other registers and him_kid_sums ran 1.2 - 1.6 %
// slower on one MI355X.  Time tools/featdist_bench.py before and after reshaping it.
__device__ __forceinline__ void gram_tile_32x32(const float* pa0, const float* pa1, const float* pb0, const float* pb1, int D,
                                                int vec, int g, mfma_d4 (&acc)[2][2]) {
  const float* const pa[2] = {pa0, pa1};
  const float* const pb[2] = {pb0, pb1};
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < D; k0 += 16) {
    const int k = k0 + 4 * g;
    double a[2][4], b[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) gram_load4(pa[u], k, D, vec != 0, a[u]), gram_load4(pb[u], k, D, vec != 0, b[u]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][j], b[v][j], acc[u][v], 0, 0, 0);
  }
}

// the `vec` of gram_tile_32x32: every row of both matrices starts 16-byte aligned
inline int gram_vec_ok(int D, const float* a, const float* b) {
  return (D % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0) ? 1 : 0;
}

}  // namespace him
