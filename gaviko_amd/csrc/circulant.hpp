// A real circular convolution along the contiguous axis as a product on the f32-input matrix cores, shared by motion.hip and kspace.hip:
//   Y = X . C,  X = 32 lines of W voxels in LDS,  C[k][w] = c[(w - k) mod W].
// The circulant is never materialised: every lane reads its element from a doubled copy of the row c in LDS.  256 threads = 4 waves; wave v
// owns line tile rt = v & 1 and the 16-column tiles t0, t0 + 2, ... with t0 = v >> 1, one f32x4 accumulator each.  With an odd number of
// column tiles the waves with t0 = 1 run one tile past the line (the doubled row is filled that far, the result is dropped).
#pragma once
#include "common.hpp"

namespace gvk {

constexpr int kCircThreads = 256;                              // every helper below is called by all threads of a workgroup of this size
constexpr int kCircWaves = kCircThreads / kWave;

// LDS line stride for a width rounded up to 16 columns.  Both operands of v_mfma_f32_16x16x4_f32 are read one dword per lane (ds_read_b32:
// 32 banks, the two 32-lane halves are served separately, so the 16 lanes x 2 k of one half must fall on 32 different banks).  The A operand
// is x[line l & 15][k = l >> 4]: bank = stride * line + k, so the stride is 2 above a multiple of 32, and at least Wk + 2.
__host__ __device__ constexpr int circulant_stride(int Wk) { return ((Wk + 31) & ~31) + 2; }

// s_c[i] = c[(i - Nk) mod N] for i < 2 Nk + 16: the circulant at offset (output index - k) + Nk, Nk = N rounded up to 16
__device__ __forceinline__ void circulant_fill_row(float* s_c, const float* __restrict__ c, int N, int Nk, int tid) {
  for (int i = tid; i < 2 * Nk + 16; i += kCircThreads) {
    int m = (i - Nk) % N;
    if (m < 0) m += N;
    s_c[i] = c[m];
  }
}

// acc[i] += X . C for the column tiles t0 + 2 i, i < nt <= NT, over k < W4 (W rounded up to 4; the columns W.. of s_x are zero).  NT is a
// template argument so that the accumulators are registers; a caller that passes nt = NT gets a product loop with no branch.
// Lane l holds A[line l & 15][k = k0 + (l >> 4)] and B[k = k0 + (l >> 4)][column l & 15] = c[(column - k) mod W].
template <int NT>
__device__ __forceinline__ void circulant_product(f32x4 (&acc)[NT], int nt, const float* s_x, int S, const float* s_c, int Wk, int W4, int rt, int t0,
                                                  int lane) {
  const float* xa = s_x + (rt * 16 + (lane & 15)) * S + (lane >> 4);
  const float* cb = s_c + t0 * 16 + (lane & 15) - (lane >> 4) + Wk;
  for (int k0 = 0; k0 < W4; k0 += 4) {
    const float a = xa[k0];
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (i < nt) acc[i] = mfma4(a, cb[i * 32 - k0], acc[i]);
  }
}

// The accumulators go through LDS (over the operand lines, once every wave is done with them), so that lines leave as whole rows: one dword
// per lane, 256 contiguous bytes per wave instruction (lines start on a 16-byte boundary only when W is a multiple of 4).
template <int NT>
__device__ __forceinline__ void circulant_store_lines(const f32x4 (&acc)[NT], int nt, float* s_x, int S, float* __restrict__ dst, int line0, int nlines,
                                                      int W, int Wk, int rt, int t0, int wave, int lane) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int ct = t0 + 2 * i;
    if (i < nt && ct < (Wk >> 4))                              // wave-uniform
#pragma unroll
      for (int e = 0; e < 4; ++e) s_x[(rt * 16 + (lane >> 4) * 4 + e) * S + ct * 16 + (lane & 15)] = acc[i][e];
  }
  __syncthreads();
  for (int r = wave; r < nlines; r += kCircWaves)
    for (int w = lane; w < W; w += 64) dst[(size_t)(line0 + r) * W + w] = s_x[r * S + w];
}

}  // namespace gvk
