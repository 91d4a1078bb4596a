// Resampling arithmetic shared by the kernels that read a volume at computed positions (through a 3x4 map: augment.hip,
// gvk_spatial_transform, and motion.hip, gvk_motion_artifact; through a displacement field: elastic.hip, gvk_elastic_deform) and the reduction of the volume_minmax partials that gives them their pad value.  One definition, so all of them
// round exactly alike: the spatial transform's pinned bits are this function's.
#pragma once
#include "common.hpp"

namespace gvk {

constexpr int kMmSlabs = 256;     // partial (min, max) pairs per volume (= the block size of the kernels that reduce them)

// every thread of a 256-thread block calls this (block-uniform): thread t brings partial t, the block reduces through LDS
__device__ __forceinline__ void reduce_partials(const float* part, int b, float& lo, float& hi) {
  __shared__ float rlo[256], rhi[256];
  const int tid = threadIdx.x;
  rlo[tid] = part[((size_t)b * kMmSlabs + tid) * 2];
  rhi[tid] = part[((size_t)b * kMmSlabs + tid) * 2 + 1];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { rlo[tid] = fminf(rlo[tid], rlo[tid + s]); rhi[tid] = fmaxf(rhi[tid], rhi[tid + s]); }
    __syncthreads();
  }
  lo = rlo[0]; hi = rhi[0];
}

// src [D][H][W] read at the position (pz, py, px) in voxels (array-axis order: axis 0 = depth), trilinear; neighbours outside the volume
// read `pad`
__device__ __forceinline__ float trilinear_at(const float* __restrict__ src, float pz, float py, float px, int D, int H, int W, float pad) {
  const float fz = floorf(pz), fy = floorf(py), fx = floorf(px);
  const int iz = (int)fz, iy = (int)fy, ix = (int)fx;
  const float wz = pz - fz, wy = py - fy, wx = px - fx;
  float acc = 0.f;
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int zz = iz + dz, yy = iy + dy, xx = ix + dx;
        const bool ok = zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float v = ok ? src[((size_t)zz * H + yy) * W + xx] : pad;
        const float w = (dz ? wz : 1.f - wz) * (dy ? wy : 1.f - wy) * (dx ? wx : 1.f - wx);
        acc += w * v;
      }
  return acc;
}

// src sampled at p = A q + t (m = row-major 3x4 [A | t], array-axis order)
__device__ __forceinline__ float trilinear_sample(const float* __restrict__ src, const float* __restrict__ m, float qz, float qy, float qx, int D, int H,
                                                  int W, float pad) {
  const float pz = m[0] * qz + m[1] * qy + m[2] * qx + m[3];
  const float py = m[4] * qz + m[5] * qy + m[6] * qx + m[7];
  const float px = m[8] * qz + m[9] * qy + m[10] * qx + m[11];
  return trilinear_at(src, pz, py, px, D, H, W, pad);
}

}  // namespace gvk
