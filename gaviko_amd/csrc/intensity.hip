// Intensity augmentation on the device: the intensity group train.py:43-48 declares (tio.RandomNoise, tio.RandomBiasField,
// tio.RandomBlur; RandomMotion, the fourth, is csrc/motion.hip) applied to a batch of fp32 volumes [B][D][H][W] already in HBM.
// Every kernel takes per-sample parameters, so one launch serves a batch in which each sample drew a different transform or none.
// torchio (0.20.16, requirements.txt:6) is not installed in this image: the arithmetic follows its published algorithm and is pinned
// against scipy.ndimage.gaussian_filter and a numpy restatement (tests/intensity_ref.py) -- parity with torchio itself is unpinned
// (DESIGN 8), as for RandomAffine.  All kernels are HBM-bound streams: 12.3 MB per (120,160,160) volume and pass.
#include "common.hpp"
#include "dropout.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kBlurR = GVK_BLUR_MAX_RADIUS;        // radius cap: sigma <= 4 at truncate = 4.0 gives int(16.5) = 16
constexpr int kBlurTaps = 2 * kBlurR + 1;          // row length of the weight table
constexpr int kTH = 32, kTW = 64;                  // output tile of the H/W pass
constexpr int kZChunk = 40, kZUnroll = 8;          // D pass: outputs per thread, incoming planes loaded together

// scipy mode='reflect' (d c b a | a b c d | d c b a): period 2n, mirrored in the second half; any i, so a radius above n reflects twice
__device__ __forceinline__ int reflect_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// the launch's max_radius (<= kBlurR, checked on the host) sizes LDS and the instantiations: a table entry above it is clamped, never followed
__device__ __forceinline__ int blur_radius(const int* radius, int b, int axis, int cap) { return min(max(radius[b * 3 + axis], 0), cap); }

// pass 1: the H and W axes of one z-slice tile through LDS.  (32 + 2 ry) x (64 + 2 rx) inputs with reflected halo -> W axis on every
// staged row -> H axis on the 32 output rows.  Waves take rows, lanes take columns: every LDS access is 64 consecutive words.
// Dynamic LDS, sized by the launch's largest radius m: weights, then (32 + 2m) x (64 + 2m) inputs, then (32 + 2m) x 64 W-blurred rows.
constexpr int kBlurWeightWords = (2 * kBlurTaps + 3) & ~3;
static size_t blur_hw_lds_bytes(int m) { return sizeof(float) * (kBlurWeightWords + (size_t)(kTH + 2 * m) * (kTW + 2 * m) + (size_t)(kTH + 2 * m) * kTW); }

__global__ __launch_bounds__(256) void blur_hw_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ weights,
                                                      const int* __restrict__ radius, int max_radius, int D, int H, int W, int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) float blur_lds[];
  const int kInCols = kTW + 2 * max_radius;
  float (*s_w)[kBlurTaps] = (float (*)[kBlurTaps])blur_lds;
  float* s_in = blur_lds + kBlurWeightWords;
  float* s_mid = s_in + (kTH + 2 * max_radius) * kInCols;
  const int b = blockIdx.z, z = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTW, y0 = ty * kTH;
  const int ry = blur_radius(radius, b, 1, max_radius), rx = blur_radius(radius, b, 2, max_radius);
  const int rows = kTH + 2 * ry, cols = kTW + 2 * rx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kBlurTaps) {
    s_w[0][threadIdx.x] = weights[((size_t)b * 3 + 1) * kBlurTaps + threadIdx.x];
    s_w[1][threadIdx.x] = weights[((size_t)b * 3 + 2) * kBlurTaps + threadIdx.x];
  }
  const float* src = in + ((size_t)b * D + z) * H * W;
  float* dst = out + ((size_t)b * D + z) * H * W;
  for (int row = wave; row < rows; row += 4) {
    const float* line = src + (size_t)reflect_index(y0 + row - ry, H) * W;
    for (int col = lane; col < cols; col += 64) s_in[row * kInCols + col] = line[reflect_index(x0 + col - rx, W)];
  }
  __syncthreads();
  for (int row = wave; row < rows; row += 4) {
    const float* p = s_in + row * kInCols + lane;
    float acc = s_w[1][0] * p[0];                              // first product, not 0 + ...: radius 0 (weight 1) returns the input's bits
    for (int k = 1; k <= 2 * rx; ++k) acc = __builtin_fmaf(s_w[1][k], p[k], acc);
    s_mid[row * kTW + lane] = acc;
  }
  __syncthreads();
  const int x = x0 + lane;
  for (int r = wave; r < kTH; r += 4) {
    const int y = y0 + r;
    if (y < H && x < W) {
      const float* p = s_mid + r * kTW + lane;
      float acc = s_w[0][0] * p[0];
      for (int k = 1; k <= 2 * ry; ++k) acc = __builtin_fmaf(s_w[0][k], p[k * kTW], acc);
      dst[(size_t)y * W + x] = acc;
    }
  }
}

// pass 2: the D axis as a sliding window of 2R+1 registers down one (y, x) column per lane (coalesced across the wave); a thread owns
// kZChunk outputs and loads kZUnroll incoming planes at a time so that their latencies overlap.  R is a template argument: a window
// indexed at run time would live in scratch memory.
template <int R>
__device__ __forceinline__ void blur_d_body(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ w, int D, size_t HW,
                                            int z0, int z1) {
  float wk[2 * R + 1], win[2 * R + 1];
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) wk[k] = w[k];
#pragma unroll
  for (int j = 0; j < 2 * R; ++j) win[j] = src[(size_t)reflect_index(z0 + j - R, D) * HW];
  for (int z = z0; z < z1; z += kZUnroll) {
    float nw[kZUnroll];
#pragma unroll
    for (int u = 0; u < kZUnroll; ++u) nw[u] = src[(size_t)reflect_index(z + u + R, D) * HW];
#pragma unroll
    for (int u = 0; u < kZUnroll; ++u) {
      win[2 * R] = nw[u];
      float acc = wk[0] * win[0];
#pragma unroll
      for (int k = 1; k <= 2 * R; ++k) acc = __builtin_fmaf(wk[k], win[k], acc);
      if (z + u < z1) dst[(size_t)(z + u) * HW] = acc;
#pragma unroll
      for (int k = 0; k < 2 * R; ++k) win[k] = win[k + 1];
    }
  }
}

__global__ __launch_bounds__(256) void blur_d_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ weights,
                                                     const int* __restrict__ radius, int max_radius, int D, long long HW) {
  const int b = blockIdx.z;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int z0 = blockIdx.y * kZChunk, z1 = min(D, z0 + kZChunk);
  const float* src = in + (size_t)b * D * HW + p;
  float* dst = out + (size_t)b * D * HW + p;
  const float* w = weights + (size_t)b * 3 * kBlurTaps;
  switch (blur_radius(radius, b, 0, max_radius)) {                          // block-uniform
#define GVK_BLUR_CASE(R) case R: blur_d_body<R>(src, dst, w, D, (size_t)HW, z0, z1); break;
    GVK_BLUR_CASE(0) GVK_BLUR_CASE(1) GVK_BLUR_CASE(2) GVK_BLUR_CASE(3) GVK_BLUR_CASE(4) GVK_BLUR_CASE(5) GVK_BLUR_CASE(6) GVK_BLUR_CASE(7)
    GVK_BLUR_CASE(8) GVK_BLUR_CASE(9) GVK_BLUR_CASE(10) GVK_BLUR_CASE(11) GVK_BLUR_CASE(12) GVK_BLUR_CASE(13) GVK_BLUR_CASE(14)
    GVK_BLUR_CASE(15) GVK_BLUR_CASE(16)
#undef GVK_BLUR_CASE
    default: break;
  }
}
static_assert(kBlurR == 16, "blur_d_kernel lists the radii 0..16");

// z(i) of tio.RandomNoise: Box-Muller on the counter hash of dropout.hpp.  Both uniforms are multiples of 2^-24 (exact in fp32), u1 in
// (0, 1], u2 in [0, 1); libm-grade logf / sqrtf / cosf, so a host restatement in float64 agrees to a few 1e-6 (tests/intensity_ref.py).
__device__ __forceinline__ float noise_z(unsigned long long seed, unsigned long long i) {
  const float u1 = (float)((hash_u32(seed, 2ull * i) >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(hash_u32(seed, 2ull * i + 1ull) >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// P(c0, c1, c2) of tio.RandomBiasField: sum of coeff[j] c0^a c1^b c2^c over a in 0..ORDER, b in 0..ORDER-a, c in 0..ORDER-a-b, j counting up
template <int ORDER>
__device__ __forceinline__ float bias_poly(const float* __restrict__ coeff, float c0, float c1, float c2) {
  const float p0[4] = {1.f, c0, c0 * c0, c0 * c0 * c0}, p1[4] = {1.f, c1, c1 * c1, c1 * c1 * c1}, p2[4] = {1.f, c2, c2 * c2, c2 * c2 * c2};
  float P = 0.f;
  int j = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (a + bb + c <= ORDER) P = __builtin_fmaf(coeff[j++], (p0[a] * p1[bb]) * p2[c], P);
  return P;
}
__device__ __forceinline__ float bias_field(const float* __restrict__ coeff, int order, float c0, float c1, float c2) {
  float P;
  switch (order) {                                              // launch-uniform
    case 0: P = bias_poly<0>(coeff, c0, c1, c2); break;
    case 1: P = bias_poly<1>(coeff, c0, c1, c2); break;
    case 2: P = bias_poly<2>(coeff, c0, c1, c2); break;
    default: P = bias_poly<3>(coeff, c0, c1, c2); break;
  }
  return expf(P);
}
// ck = (k - (n-1)/2) / ((n-1)/2), 0 on an axis of one voxel
__device__ __forceinline__ float bias_coord(int k, int n) {
  const float h = 0.5f * (float)(n - 1);
  return n > 1 ? ((float)k - h) / h : 0.f;
}

// one streaming pass, 16 bytes per lane; kind[b]: 0 copy, 1 noise y = x + (std z(i) + mean), 2 bias field y = x exp(P)
__global__ __launch_bounds__(256) void intensity_pointwise_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ kind,
                                                                  const float* __restrict__ noise, const unsigned long long* __restrict__ seeds,
                                                                  const float* __restrict__ coeff, int order, int D, int H, int W) {
  const int b = blockIdx.y;
  const int V = D * H * W, V4 = V >> 2, HW = H * W;
  const f32x4* x4 = (const f32x4*)(x + (size_t)b * V);
  f32x4* y4 = (f32x4*)(y + (size_t)b * V);
  const int kd = kind[b];
  const int step = gridDim.x * 256;
  if (kd == 1) {
    const float sd = noise[2 * b], mean = noise[2 * b + 1];
    const unsigned long long seed = seeds[b];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V4; i += step) {
      f32x4 v = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = sd * noise_z(seed, (unsigned long long)(4 * i + e));
        t = t + mean;
        v[e] = v[e] + t;
      }
      y4[i] = v;
    }
  } else if (kd == 2) {
    const float* cf = coeff + (size_t)b * GVK_BIAS_COEFFS;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V4; i += step) {
      f32x4 v = x4[i];
      const int i0 = 4 * i;
      int pz = i0 / HW;
      const int rem = i0 - pz * HW;
      int py = rem / W, px = rem - py * W;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = v[e] * bias_field(cf, order, bias_coord(pz, D), bias_coord(py, H), bias_coord(px, W));
        if (++px == W) {
          px = 0;
          if (++py == H) { py = 0; ++pz; }
        }
      }
      y4[i] = v;
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V4; i += step) y4[i] = x4[i];
  }
}

}  // namespace gvk

extern "C" int gvk_gaussian_blur3d(const float* in, float* out, float* scratch, const float* weights, const int32_t* radius, int max_radius, int B,
                                   int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && scratch && weights && radius, "gvk_gaussian_blur3d: null pointer");
  GVK_REQUIRE(in != out && in != scratch && out != scratch, "gvk_gaussian_blur3d: in, out and scratch must be three different buffers");
  GVK_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535 && D <= 65535, "gvk_gaussian_blur3d: bad shape");
  GVK_REQUIRE((int64_t)D * H * W < (1ll << 31), "gvk_gaussian_blur3d: volumes of 2^31 voxels or more are not built");
  GVK_REQUIRE(max_radius >= 0 && max_radius <= kBlurR,
              "gvk_gaussian_blur3d: radius %d exceeds %d -- sigma above 4 (radius int(4 sigma + 0.5) above 16) is not built", max_radius, kBlurR);
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const int64_t HW = (int64_t)H * W;
  hipStream_t s = (hipStream_t)stream;
  GVK_LAUNCH(blur_hw_kernel, dim3(tiles_x * tiles_y, D, B), dim3(256), (unsigned)blur_hw_lds_bytes(max_radius), s, in, scratch, weights,
             (const int*)radius, max_radius, D, H, W, tiles_x);
  GVK_LAUNCH(blur_d_kernel, dim3((unsigned)((HW + 255) / 256), (D + kZChunk - 1) / kZChunk, B), dim3(256), 0, s, (const float*)scratch, out, weights,
             (const int*)radius, max_radius, D, (long long)HW);
  return check_launch("gaussian_blur3d");
}

extern "C" int gvk_intensity_pointwise(const float* x, float* y, const int32_t* kind, const float* noise, const void* seeds, const float* coeff, int order,
                                       int B, int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && y && kind && noise && seeds && coeff, "gvk_intensity_pointwise: null pointer");
  GVK_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "gvk_intensity_pointwise: bad shape");
  GVK_REQUIRE(order >= 0 && order <= 3, "gvk_intensity_pointwise: bias-field order %d (0..3 are built)", order);
  const int64_t V = (int64_t)D * H * W;
  GVK_REQUIRE(V < (1ll << 31), "gvk_intensity_pointwise: volumes of 2^31 voxels or more are not built");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && V % 4 == 0, "gvk_intensity_pointwise: 16-byte aligned volumes, V a multiple of 4");
  const int gx = (int)std::min<int64_t>((V / 4 + 255) / 256, 1024);
  GVK_LAUNCH(intensity_pointwise_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, y, (const int*)kind, noise, (const unsigned long long*)seeds,
             coeff, order, D, H, W);
  return check_launch("intensity_pointwise");
}
