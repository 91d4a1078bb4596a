// Raw volumes of any shape and spacing onto the model grid (gaviko_amd.data.Conform): torchio's first stage -- Resample to a spacing or
// Resize, then CropOrPad -- for a ragged batch.  The output grid is the same for every sample, only the reads are ragged, so one launch
// sequence turns a packed buffer of unequal volumes into the batch tensor [B][D][H][W].  All geometry (edge-aligned positions, linear or
// nearest taps, the antialiasing Gaussian composed into them, crop and pad offsets) is folded on the host into one banded table per sample
// and axis (include/gaviko_hip.h); the kernels only gather and contract.  torchio and SimpleITK are not installed here: the definitions are
// this package's own and parity with torchio is unpinned.
// The contraction is separable and runs as up to three streaming passes, one contracted axis each, the axis of largest reduction first, so
// that the float32 intermediates are as small as they can be; lanes run along W in every pass.
#include "common.hpp"
#include "resample.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kConformZ = 8;      // output planes per workgroup (64 x 4 voxels of each)

// per-sample (min, max) of a packed buffer: slab x sample -> one pair, the layout reduce_partials reads.  Sample starts have no alignment,
// so the loads are scalar (four independent ones in flight per lane).
__global__ __launch_bounds__(256) void ragged_minmax_kernel(const float* __restrict__ data, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ counts, float* __restrict__ part) {
  __shared__ float smin[256], smax[256];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const long long V = counts[b];
  const float* x = data + offsets[b];
  const long long per = (V + kMmSlabs - 1) / kMmSlabs;
  const long long i0 = slab * per, i1 = min(V, i0 + per);
  float lo = INFINITY, hi = -INFINITY;
  long long i = i0 + tid;
  for (; i + 768 < i1; i += 1024) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = x[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u) { lo = fminf(lo, v[u]); hi = fmaxf(hi, v[u]); }
  }
  for (; i < i1; i += 256) {
    const float v = x[i];
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  smin[tid] = lo; smax[tid] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { smin[tid] = fminf(smin[tid], smin[tid + s]); smax[tid] = fmaxf(smax[tid], smax[tid + s]); }
    __syncthreads();
  }
  if (tid == 0) { part[((size_t)b * kMmSlabs + slab) * 2] = smin[0]; part[((size_t)b * kMmSlabs + slab) * 2 + 1] = smax[0]; }
}

// one pass: a workgroup writes 64 (x) x 4 (y) x kConformZ (z) voxels of one sample's output of this pass.  Axis modes (meta row): 0 untouched,
// 1 gathered here, 2 contracted here, 3 done earlier.  A voxel outside on any touched axis is the pad value, whatever was read before.
__global__ __launch_bounds__(256) void conform_pass_kernel(gvk_conform_desc d, int pass, int zchunks) {
  const int b = blockIdx.z / zchunks, zc = blockIdx.z - b * zchunks;
  const int32_t* __restrict__ m = d.meta + ((size_t)pass * d.B + b) * GVK_CONFORM_META;
  if (!m[0]) return;                                           // block-uniform: the sample finished in an earlier pass
  float pad = d.pad_value;
  if (d.pad_min) { float hi_unused; reduce_partials(d.partials, b, pad, hi_unused); }      // block-uniform, before any thread leaves
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int o0 = m[9], o1 = m[10], o2 = m[11];
  const int z0 = zc * kConformZ, z1 = min(z0 + kConformZ, o0);
  if (x >= o2 || y >= o1 || z0 >= o0) return;
  const int mode0 = m[3], mode1 = m[4], mode2 = m[5], n1 = m[7], n2 = m[8], ca = m[12], K = m[13], T = d.T;
  const size_t rb = (size_t)b * (d.D + d.H + d.W), r1 = rb + d.D + y, r2 = rb + d.D + d.H + x;
  int i1 = y, i2 = x;
  bool outside = false;
  if (mode1) { outside |= !d.inside[r1]; if (mode1 != 3) i1 = d.start[r1]; }
  if (mode2) { outside |= !d.inside[r2]; if (mode2 != 3) i2 = d.start[r2]; }
  const float* __restrict__ src = (m[1] ? d.scratch : d.data) + d.src_off[(size_t)pass * d.B + b];
  float* __restrict__ dst = (m[2] ? d.out : d.scratch) + d.dst_off[(size_t)pass * d.B + b];
  const size_t plane = (size_t)n1 * n2;
  const size_t stride = ca == 0 ? plane : ca == 1 ? (size_t)n2 : 1;
  const float* __restrict__ wrow = d.weights + (ca == 1 ? r1 : r2) * T;      // replaced per plane when axis 0 is the contracted one
  for (int z = z0; z < z1; ++z) {
    int i0 = z;
    bool out0 = false;
    if (mode0) { out0 = !d.inside[rb + z]; if (mode0 != 3) i0 = d.start[rb + z]; }
    float v = pad;
    if (!(outside || out0)) {
      const float* __restrict__ p = src + ((size_t)i0 * n1 + i1) * n2 + i2;
      if (ca < 0) {
        v = p[0];                                              // a move of bits
      } else {
        const float* __restrict__ w = ca == 0 ? d.weights + (rb + z) * T : wrow;
        v = w[0] * p[0];
        for (int t = 1; t < K; ++t) v = __builtin_fmaf(w[t], p[t * stride], v);
      }
    }
    dst[((size_t)z * o1 + y) * o2 + x] = v;
  }
}

}  // namespace gvk

extern "C" int gvk_ragged_minmax(const float* data, const int64_t* offsets, const int64_t* counts, float* partials, int B, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(data && offsets && counts && partials && B > 0 && B <= 65535, "gvk_ragged_minmax: bad arguments");
  GVK_LAUNCH(ragged_minmax_kernel, dim3(kMmSlabs, B), dim3(256), 0, (hipStream_t)stream, data, offsets, counts, partials);
  return check_launch("ragged_minmax");
}

extern "C" int gvk_conform_volumes(const gvk_conform_desc* dp, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(dp, "gvk_conform_volumes: null descriptor");
  const gvk_conform_desc d = *dp;
  GVK_REQUIRE(d.data && d.out && d.src_off && d.dst_off && d.meta && d.start && d.inside && d.weights, "gvk_conform_volumes: null pointer");
  GVK_REQUIRE(d.B > 0 && d.D > 0 && d.H > 0 && d.W > 0, "gvk_conform_volumes: bad shape");
  GVK_REQUIRE(d.T >= 1 && d.T <= GVK_CONFORM_MAX_TAPS, "gvk_conform_volumes: 1..%d taps per table row, not %d", (int)GVK_CONFORM_MAX_TAPS, d.T);
  GVK_REQUIRE(d.npass >= 1 && d.npass <= 3, "gvk_conform_volumes: 1..3 passes, not %d", d.npass);
  GVK_REQUIRE(d.npass == 1 || d.scratch, "gvk_conform_volumes: more than one pass needs the scratch buffer");
  GVK_REQUIRE(!d.pad_min || d.partials, "gvk_conform_volumes: pad_min needs the partials of gvk_ragged_minmax");
  GVK_REQUIRE(d.data != d.out && d.scratch != d.out && d.scratch != d.data, "gvk_conform_volumes: data, scratch and out must be distinct buffers");
  const int dims[3][3] = {{d.p0d0, d.p0d1, d.p0d2}, {d.p1d0, d.p1d1, d.p1d2}, {d.p2d0, d.p2d1, d.p2d2}};
  for (int p = 0; p < d.npass; ++p) {
    GVK_REQUIRE(dims[p][0] > 0 && dims[p][1] > 0 && dims[p][2] > 0, "gvk_conform_volumes: pass %d has an empty grid", p);
    const long long zchunks = (dims[p][0] + kConformZ - 1) / kConformZ, gy = (dims[p][1] + 3) / 4;
    GVK_REQUIRE(zchunks * d.B <= 65535 && gy <= 65535, "gvk_conform_volumes: pass %d needs a grid of %lld x %lld (y, z), at most 65535 each", p, gy,
                zchunks * d.B);
  }
  for (int p = 0; p < d.npass; ++p) {
    const int zchunks = (dims[p][0] + kConformZ - 1) / kConformZ;
    GVK_LAUNCH(conform_pass_kernel, dim3((dims[p][2] + 63) / 64, (dims[p][1] + 3) / 4, zchunks * d.B), dim3(256), 0, (hipStream_t)stream, d, p, zchunks);
  }
  return check_launch("conform_volumes");
}
