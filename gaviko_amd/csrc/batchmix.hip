// Mixup and CutMix on the device (timm.data.Mixup's arithmetic on a batch of volumes): the first transform here that combines TWO samples.
// One streaming pass, one launch per batch whatever the mix of modes; x, out float32 [B][V], V = D*H*W < 2^31, out must not overlap x.
// Per sample b, with partner p = perm[b]:
//   GVK_MIX_COPY    out[b] = x[b], bit for bit; lam, perm and box are not read
//   GVK_MIX_MIXUP   out[b] = lam[b] * x[b] + (1 - lam[b]) * x[p] in float32, 1 - lam[b] formed here in float32.  The TWO-ROUNDING form: each
//                   product is rounded, then the sum (the library builds with -ffp-contract=off).  A term whose coefficient is exactly 0 is
//                   left out and its volume is not read: lam = 1 gives x[b] and lam = 0 gives x[p] bit for bit (0 * x would turn -0 into +0
//                   and an infinity into NaN).
//   GVK_MIX_CUTMIX  box[b] = (d0, d1, h0, h1, w0, w1), half-open: out[b] = x[p] inside the box, x[b] outside, bit for bit; lam is not read.
//                   An empty box is the copy of x[b], a box that covers the volume the copy of x[p].
// So a sample comes down to one of three forms: copy of ONE source (x[b] or x[p]), the two-source sum, or the box select -- copy and CutMix
// read one source voxel per output voxel, Mixup two.  A sample is cut into 16-byte groups of four voxels when every address it touches is on
// the 16-byte grid (out + b V, and the sources it reads: with V odd every second sample is off it) and runs the same arithmetic voxel by voxel
// otherwise; the V % 4 voxels after the last group are scalar.  Under CutMix a group that lies in one W-row wholly outside or wholly inside
// the box's w-range is one 16-byte load from that source; a group the box's edge (or a row's end, when W is no multiple of 4) cuts is four
// scalar loads, each from its own source.  No atomics, no LDS: every output voxel is written once by one thread.
#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kMixSlabs = 512;                                   // workgroups per sample, at most: 8 per CU at B = 4
constexpr int kMixUnroll = 4;                                    // independent 16-byte loads in flight per lane and source

struct MixBox { int d0, d1, h0, h1, w0, w1; };

__device__ __forceinline__ bool in_box(const MixBox& q, int d, int h, int w) {
  return d >= q.d0 && d < q.d1 && h >= q.h0 && h < q.h1 && w >= q.w0 && w < q.w1;
}

// one output voxel: form 0 = s0[i], 1 = ca s0[i] + cb s1[i], 2 = the box select between s0 (outside) and s1 (inside)
__device__ __forceinline__ float mix_one(const float* __restrict__ s0, const float* __restrict__ s1, int form, float ca, float cb, const MixBox& q,
                                         unsigned i, unsigned H, unsigned W) {
  if (form == 1) return ca * s0[i] + cb * s1[i];
  const float* s = s0;
  if (form == 2) {
    const unsigned row = i / W, w = i - row * W, d = row / H, h = row - d * H;
    if (in_box(q, (int)d, (int)h, (int)w)) s = s1;
  }
  return s[i];
}

__global__ __launch_bounds__(256) void batch_mix_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ mode,
                                                        const float* __restrict__ lam, const int* __restrict__ perm, const int* __restrict__ box,
                                                        unsigned V, int B, int D, int H, int W) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m = mode[b];
  const float* s0 = x + (size_t)b * V;
  const float* s1 = s0;
  float* ob = out + (size_t)b * V;
  int form = 0;
  float ca = 1.f, cb = 0.f;
  MixBox q = {0, 0, 0, 0, 0, 0};
  if (m == GVK_MIX_MIXUP || m == GVK_MIX_CUTMIX) {
    int p = perm[b];
    p = p < 0 ? 0 : (p >= B ? B - 1 : p);                        // the caller's contract; clamped so that nothing outside x is read
    s1 = x + (size_t)p * V;
    if (m == GVK_MIX_MIXUP) {
      ca = lam[b];
      cb = 1.f - ca;
      if (ca == 0.f) s0 = s1;                                    // only the partner counts
      else if (cb != 0.f) form = 1;
    } else {
      const int* bx = box + (size_t)b * 6;
      q = {max(bx[0], 0), min(bx[1], D), max(bx[2], 0), min(bx[3], H), max(bx[4], 0), min(bx[5], W)};
      const bool empty = q.d1 <= q.d0 || q.h1 <= q.h0 || q.w1 <= q.w0;
      const bool full = q.d0 == 0 && q.d1 == D && q.h0 == 0 && q.h1 == H && q.w0 == 0 && q.w1 == W;
      if (full) s0 = s1;
      else if (!empty) form = 2;
    }
  }
  const bool two = form != 0;                                    // form 0 reads s0 alone
  const bool wide = ((((uintptr_t)ob | (uintptr_t)s0 | (two ? (uintptr_t)s1 : (uintptr_t)0)) & 15) == 0);
  if (!wide) {                                                   // off the 16-byte grid: the same arithmetic voxel by voxel, lanes along W
#pragma unroll 1
    for (unsigned i = blockIdx.x * 256u + tid; i < V; i += gridDim.x * 256u) ob[i] = mix_one(s0, s1, form, ca, cb, q, i, (unsigned)H, (unsigned)W);
    return;
  }
  const unsigned n4 = V >> 2;
  const f32x4* a4 = (const f32x4*)s0;
  const f32x4* p4 = (const f32x4*)s1;
  f32x4* o4 = (f32x4*)ob;
  const unsigned first = blockIdx.x * 256u * kMixUnroll + tid, step = gridDim.x * 256u * kMixUnroll;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (form == 0) {                                               // one loop per form: the form is the workgroup's, not the voxel's
    for (unsigned base = first; base < n4 + tid; base += step) {
      f32x4 v[kMixUnroll];
#pragma unroll
      for (int u = 0; u < kMixUnroll; ++u) v[u] = base + 256u * u < n4 ? a4[base + 256u * u] : zero;
#pragma unroll
      for (int u = 0; u < kMixUnroll; ++u)
        if (base + 256u * u < n4) o4[base + 256u * u] = v[u];
    }
  } else if (form == 1) {
    for (unsigned base = first; base < n4 + tid; base += step) {
      f32x4 v[kMixUnroll], r[kMixUnroll];
#pragma unroll
      for (int u = 0; u < kMixUnroll; ++u) {
        const bool ok = base + 256u * u < n4;
        v[u] = ok ? a4[base + 256u * u] : zero;
        r[u] = ok ? p4[base + 256u * u] : zero;
      }
#pragma unroll
      for (int u = 0; u < kMixUnroll; ++u) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = ca * v[u][e] + cb * r[u][e];
        if (base + 256u * u < n4) o4[base + 256u * u] = y;
      }
    }
  } else {
#pragma unroll 1
    for (unsigned i = blockIdx.x * 256u + tid; i < n4; i += gridDim.x * 256u) {
      const unsigned f = i << 2, row = f / (unsigned)W, w = f - row * (unsigned)W;
      f32x4 y;
      if (w + 4u <= (unsigned)W) {                               // the group lies in one W-row
        const unsigned d = row / (unsigned)H, h = row - d * (unsigned)H;
        const bool rin = (int)d >= q.d0 && (int)d < q.d1 && (int)h >= q.h0 && (int)h < q.h1;
        if (!rin || (int)w + 4 <= q.w0 || (int)w >= q.w1) y = a4[i];
        else if ((int)w >= q.w0 && (int)w + 4 <= q.w1) y = p4[i];
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = ((int)w + e >= q.w0 && (int)w + e < q.w1) ? s1[f + e] : s0[f + e];
        }
      } else {                                                   // a row ends inside the group (W is no multiple of 4)
#pragma unroll 1
        for (int e = 0; e < 4; ++e) y[e] = mix_one(s0, s1, 2, ca, cb, q, f + e, (unsigned)H, (unsigned)W);
      }
      o4[i] = y;
    }
  }
  const unsigned t = (n4 << 2) + tid;                            // the V % 4 voxels after the last group
  if (blockIdx.x == 0 && t < V) ob[t] = mix_one(s0, s1, form, ca, cb, q, t, (unsigned)H, (unsigned)W);
}

}  // namespace gvk

extern "C" int gvk_batch_mix(const float* x, float* out, const int32_t* mode, const float* lam, const int32_t* perm, const int32_t* box, int B, int D,
                             int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && out && mode && lam && perm && box, "gvk_batch_mix: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && D > 0 && H > 0 && W > 0, "gvk_batch_mix: B=%d D=%d H=%d W=%d", B, D, H, W);
  const int64_t V = (int64_t)D * H * W;
  GVK_REQUIRE(V < ((int64_t)1 << 31), "gvk_batch_mix: D*H*W must be below 2^31");
  GVK_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0, "gvk_batch_mix: x and out must be float-aligned");
  const int64_t bytes = (int64_t)B * V * 4;
  GVK_REQUIRE((const char*)out + bytes <= (const char*)x || (const char*)x + bytes <= (const char*)out, "gvk_batch_mix: out must not overlap x");
  const int gx = (int)std::min<int64_t>(kMixSlabs, (V / 4 + 256 * kMixUnroll - 1) / (256 * kMixUnroll) + 1);
  GVK_LAUNCH(batch_mix_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, out, (const int*)mode, lam, (const int*)perm, (const int*)box,
             (unsigned)V, B, D, H, W);
  return check_launch("batch_mix");
}
