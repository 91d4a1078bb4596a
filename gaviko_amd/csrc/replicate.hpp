// What the resampling evaluation kernels share (bootstrap.hip, selective.hip, conformal.hip, roc.hip): one 256-thread workgroup per replicate b,
// the replicate drawn from hash_u32(seed, b N + n), and an inclusive scan over the sorted positions held in LDS.
#pragma once
#include "common.hpp"
#include "dropout.hpp"

namespace gvk {

constexpr int kScanTile = 1024;                                  // scan tile: 256 threads x 4 consecutive entries (one 16-byte LDS access each)
inline int scan_pad(int N) { return (N + kScanTile - 1) / kScanTile * kScanTile; }   // the Npad of the kernels: N rounded up to the scan tile

// an index or a label read from a table or from the caller, brought inside the array it addresses
__device__ __forceinline__ int clamp_row(int row, int N) { return row < 0 ? 0 : (row >= N ? N - 1 : row); }
__device__ __forceinline__ int clamp_label(long long y, int K) { return y < 0 ? 0 : (y >= K ? K - 1 : (int)y); }

// The row that draw n of replicate b takes (include/gaviko_hip.h states the two rules).  plain: (h N) >> 32, below N because h < 2^32.
// stratified: the ((h n_c) >> 32)-th row of the class c of row n; class_off / class_rows are the caller's tables, so both reads are clamped.
__device__ __forceinline__ int draw_row(unsigned long long seed, unsigned long long b, int n, int N, int K, const long long* __restrict__ labels,
                                        const int* __restrict__ class_rows, const int* __restrict__ class_off, int stratified) {
  const unsigned long long h = hash_u32(seed, b * (unsigned long long)N + (unsigned long long)n);
  if (!stratified) return (int)((h * (unsigned long long)N) >> 32);
  const int c = clamp_label(labels[n], K);
  const int o0 = class_off[c], nc = class_off[c + 1] - o0;
  const int q = clamp_row(o0 + (int)((h * (unsigned long long)(nc > 0 ? nc : 0)) >> 32), N);
  return clamp_row(class_rows[q], N);
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned int wave_scan_u32(unsigned int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// In-place inclusive scan of P[0..Npad) in LDS, Npad a multiple of kScanTile and P 16-byte aligned; returns the total.  Per tile: 4 entries
// per thread, the wave scan of the thread totals, the 4 wave totals through s_wave (4 LDS words of the caller's) and a running carry.
// Contract: all 256 threads call it in uniform control flow; the caller has put a barrier after filling P; it returns after a barrier, so P is
// complete for every thread and s_wave is free.
__device__ __forceinline__ unsigned int block_scan_tiles_u32(unsigned int* P, int Npad, unsigned int* s_wave) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned int carry = 0u;                                                  // sum of the tiles before this one: the same in every thread
  for (int s0 = 0; s0 < Npad; s0 += kScanTile) {
    u32x4 v = *(const u32x4*)(P + s0 + 4 * t);
    v.y += v.x; v.z += v.y; v.w += v.z;
    const unsigned int tot = v.w, inc = wave_scan_u32(tot);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    const unsigned int w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
    const unsigned int base = carry + (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u) + (inc - tot);
    v.x += base; v.y += base; v.z += base; v.w += base;
    *(u32x4*)(P + s0 + 4 * t) = v;
    carry += w0 + w1 + w2 + w3;
    __syncthreads();                                                        // s_wave is free for the next tile
  }
  return carry;
}

}  // namespace gvk
