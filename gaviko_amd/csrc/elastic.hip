// tio.RandomElasticDeformation on the device: a random displacement on a coarse grid of control points, interpolated to every voxel with
// cubic B-splines (ITK's order-3 BSplineTransform over the image extent, which torchio runs through SimpleITK on the CPU), and the volume
// read back through it with the trilinear arithmetic and pad rule of gvk_spatial_transform (resample.hpp) -- ONE pass over a batch of fp32
// volumes [B][D][H][W] already in HBM.
//
// Per axis with S voxels and n control points the mesh has M = n - 3 cells of h = S / M voxels; output index q lies at u = (q + 0.5) / h
// cells from the low face of the volume, in cell i = min(floor(u), M - 1) at t = u - i, and control points i..i+3 weigh
//   B0 = (1-t)^3 / 6,   B1 = (3t^3 - 6t^2 + 4) / 6,   B2 = (-3t^3 + 3t^2 + 3t + 1) / 6,   B3 = t^3 / 6        (they sum to 1).
// The displacement d(q) (voxels, component a along array axis a) is the tensor product of the three axes' weights over the 4 x 4 x 4
// control points, and out[q] = in read at float(q) + d(q).
//
// The tensor product is separable and the kernel uses that: a workgroup owns 64 voxels along W x 4 rows along H and walks down D (the
// layout of spatial_kernel); the sample's whole control grid sits in LDS (n0 n1 n2 3 floats, 49 KB at the cap of 16 per axis, 4 KB at
// torchio's default 7).  For each z, 4 rows x n2 x 3 threads each contract the z and y control indices of one (row, W-index, component)
// -- 16 multiply-adds from LDS -- into a row-coefficient table, double-buffered so that one barrier per z suffices; every voxel then takes
// its 4 taps x 3 components from that table (lanes of a row mostly share the cell: LDS broadcasts) and does its 8-neighbour gather.  Per
// voxel that is 12 multiply-adds on top of gvk_spatial_transform's work, never a 64-tap loop, and no lane reads the grid from global memory.
// No atomics, a fixed order of operations: the same bits on every run.
#include "common.hpp"
#include "resample.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kElMin = 4, kElMax = GVK_ELASTIC_MAX_CONTROL_POINTS;

// cell index and the four weights of output index q on an axis of S voxels with M mesh cells (fp32; q + 0.5 is exact below 2^23)
__device__ __forceinline__ int bspline_taps(int q, int S, int M, float w[4]) {
  const float u = ((float)q + 0.5f) * (float)M / (float)S;
  const int i = min((int)floorf(u), M - 1);
  const float t = u - (float)i, s = 1.f - t, t2 = t * t, t3 = t2 * t, sixth = 1.f / 6.f;
  w[0] = s * s * s * sixth;
  w[1] = (3.f * t3 - 6.f * t2 + 4.f) * sixth;
  w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * sixth;
  w[3] = t3 * sixth;
  return i;
}

__global__ __launch_bounds__(256) void elastic_kernel(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ field,
                                                      const float* __restrict__ ctrl, const int* __restrict__ live, const float* __restrict__ part,
                                                      int D, int H, int W, int n0, int n1, int n2) {
  extern __shared__ float s_ctrl[];                            // [n0][n1][n2][3] of this sample
  __shared__ float s_row[2][4 * kElMax * 3];                   // [z parity][row][W control index][component]
  const int b = blockIdx.z, tid = threadIdx.x;
  const int r = tid >> 6, x = blockIdx.x * 64 + (tid & 63), y = blockIdx.y * 4 + r;
  const bool inside = x < W && y < H;
  const size_t HW = (size_t)H * W, V = HW * D;
  const float* src = in + (size_t)b * V;
  float* dst = out + (size_t)b * V;
  float* fld = field ? field + (size_t)b * 3 * V : nullptr;
  if (!live[b]) {                                              // block-uniform: this sample drew nothing, its bits pass through
    if (inside)
      for (int z = 0; z < D; ++z) {
        const size_t o = z * HW + (size_t)y * W + x;
        dst[o] = src[o];
        if (fld) { fld[o] = 0.f; fld[V + o] = 0.f; fld[2 * V + o] = 0.f; }
      }
    return;
  }
  float pad, hi_unused;
  reduce_partials(part, b, pad, hi_unused);
  const int n23 = n2 * 3, nc = n0 * n1 * n23;
  for (int i = tid; i < nc; i += 256) s_ctrl[i] = ctrl[(size_t)b * nc + i];
  float wx[4];
  const int i2 = bspline_taps(min(x, W - 1), W, n2 - 3, wx);    // lanes past the row keep valid indices; they take part in the barriers only
  // thread tid < 4 n2 3 builds row coefficient kc = (W control index, component) of row rr
  const bool builder = tid < 4 * n23;
  const int rr = builder ? tid / n23 : 0, kc = tid - rr * n23;
  float wy[4];
  const int i1 = bspline_taps(min((int)blockIdx.y * 4 + rr, H - 1), H, n1 - 3, wy);
  __syncthreads();
  for (int z = 0; z < D; ++z) {
    float* row = s_row[z & 1];                                 // written two barriers after its last readers arrived at one
    if (builder) {
      float wz[4];
      const int i0 = bspline_taps(z, D, n0 - 3, wz);
      const float* c = s_ctrl + (i0 * n1 + i1) * n23 + kc;
      float acc = 0.f;
#pragma unroll
      for (int j0 = 0; j0 < 4; ++j0) {
        float a = 0.f;
#pragma unroll
        for (int j1 = 0; j1 < 4; ++j1) a = fmaf(wy[j1], c[(j0 * n1 + j1) * n23], a);
        acc = fmaf(wz[j0], a, acc);
      }
      row[rr * n23 + kc] = acc;
    }
    __syncthreads();
    if (inside) {
      const float* rc = row + (r * n2 + i2) * 3;
      float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d0 = fmaf(wx[j], rc[3 * j], d0);
        d1 = fmaf(wx[j], rc[3 * j + 1], d1);
        d2 = fmaf(wx[j], rc[3 * j + 2], d2);
      }
      const size_t o = z * HW + (size_t)y * W + x;
      dst[o] = trilinear_at(src, (float)z + d0, (float)y + d1, (float)x + d2, D, H, W, pad);
      if (fld) { fld[o] = d0; fld[V + o] = d1; fld[2 * V + o] = d2; }
    }
  }
}

}  // namespace gvk

extern "C" int gvk_elastic_deform(const float* in, float* out, float* field, const float* ctrl, const int32_t* live, const float* partials, int B, int D,
                                  int H, int W, int n0, int n1, int n2, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && ctrl && live && partials, "gvk_elastic_deform: null pointer");
  GVK_REQUIRE(std::min({n0, n1, n2}) >= kElMin && std::max({n0, n1, n2}) <= kElMax,
              "gvk_elastic_deform: %d x %d x %d control points (%d..%d per axis are built)", n0, n1, n2, kElMin, kElMax);
  GVK_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535 && std::max({D, H, W}) < (1 << 23) && (H + 3) / 4 <= 65535, "gvk_elastic_deform: bad shape");
  const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out, f = (uintptr_t)field, bytes = (uintptr_t)B * D * H * W * sizeof(float);
  GVK_REQUIRE(a + bytes <= o || o + bytes <= a, "gvk_elastic_deform: in and out must not overlap (the kernel reads neighbouring voxels)");
  GVK_REQUIRE(!field || ((f + 3 * bytes <= a || a + bytes <= f) && (f + 3 * bytes <= o || o + bytes <= f)),
              "gvk_elastic_deform: field must not overlap in or out");
  const unsigned lds = (unsigned)(n0 * n1 * n2 * 3 * sizeof(float));
  GVK_LAUNCH(elastic_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(256), lds, (hipStream_t)stream, in, out, field, ctrl, (const int*)live, partials, D,
             H, W, n0, n1, n2);
  return check_launch("elastic_deform");
}
