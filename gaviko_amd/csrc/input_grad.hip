// Input gradients (gradient saliency, gradient x input, integrated gradients) -- the last steps of a backward that reaches the voxels.
//   unpatchify     the patch embedding is a Conv3d with stride == kernel, so the gradient of its input is a pure permutation of the
//                  gradient of its im2col matrix: dcols [rows][K] -> volume, the inverse index map of patchify_kernel (elementwise.hip),
//                  with the attribution arithmetic in the same pass (alpha / beta, x (x - x0), a sum over consecutive samples).
//   patch_reduce   volume map -> one value per patch (sum of |g| or signed sum), on the patch grid of explain.patch_grid.
//   evp_highpass_sign / evp_highpass_linear   the backward of the EVP high-pass (evp.hip: out = |Hp . X| on the filtered depth slices,
//                  |X| on the others).  It is not linear (the modulus), so its adjoint is two steps: g = dout o sign(Hp . X) (sign(X) on the
//                  other slices), then dX = Hp^T . g -- the linear form with the transposed operator.
#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// out[b] = beta * out[b] + sum_{j < nsum} alpha * G[b * nsum + j] (* (x[b] - x0[b])), G = the volume of dcols rows (b * nsum + j) * N ...
// One thread per 4 consecutive voxels along W (pw % 4 == 0: they are 4 consecutive columns of one dcols row).  The sum runs over j in order
// as one FMA per step, so splitting the j range over several calls (beta = 1 after the first) gives the same bits.  beta == 0 never reads out.
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ dcols, float* __restrict__ out, const float* __restrict__ x,
                                                         const float* __restrict__ x0, int B, int D, int H, int W, int pd, int ph, int pw,
                                                         int nsum, float alpha, float beta) {
  const int nd = D / pd, nh = H / ph, nw = W / pw;
  const int K = pd * ph * pw;
  const int64_t N = (int64_t)nd * nh * nw;
  const int wq = W / 4;
  const int64_t total = (int64_t)B * D * H * wq;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    int64_t t = idx;
    const int x4 = t % wq; t /= wq;
    const int y = t % H; t /= H;
    const int z = t % D; const int b = t / D;
    const int xx = x4 * 4;
    const int d = z / pd, kd = z - d * pd, h = y / ph, kh = y - h * ph, w = xx / pw, kw = xx - w * pw;
    const int64_t n = ((int64_t)d * nh + h) * nw + w;
    const int64_t k = (kd * ph + kh) * pw + kw;
    const int64_t vo = (((int64_t)b * D + z) * H + y) * W + xx;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (beta != 0.f) acc = beta * *(const f32x4*)(out + vo);
    f32x4 dx = {1.f, 1.f, 1.f, 1.f};
    if (x != nullptr) {
      dx = *(const f32x4*)(x + vo);
      if (x0 != nullptr) dx -= *(const f32x4*)(x0 + vo);
    }
    for (int j = 0; j < nsum; ++j) {
      const f32x4 g = *(const f32x4*)(dcols + (((int64_t)b * nsum + j) * N + n) * K + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(alpha * g[e], dx[e], acc[e]);
    }
    *(f32x4*)(out + vo) = acc;
  }
}

// out[b][d][h][w] = sum over the voxels of patch (d, h, w) of |v| (absval) or v.  One workgroup per patch; every thread sums a fixed strided
// subset in order, then a fixed tree in LDS: deterministic.
__global__ __launch_bounds__(256) void patch_reduce_kernel(const float* __restrict__ vol, float* __restrict__ out, int D, int H, int W, int pd,
                                                           int ph, int pw, int absval) {
  __shared__ float red[256];
  const int nd = D / pd, nh = H / ph, nw = W / pw;
  const int64_t p = blockIdx.x;                        // (b, d, h, w) in grid order
  const int w = p % nw, h = (p / nw) % nh, d = (p / ((int64_t)nw * nh)) % nd;
  const int64_t b = p / ((int64_t)nw * nh * nd);
  const int pq = pw / 4, rows = pd * ph;
  float s = 0.f;
  for (int i = threadIdx.x; i < rows * pq; i += 256) {
    const int r = i / pq, c = (i - r * pq) * 4;
    const int z = d * pd + r / ph, y = h * ph + r % ph;
    const f32x4 v = *(const f32x4*)(vol + ((b * D + z) * H + y) * W + w * pw + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += absval ? fabsf(v[e]) : v[e];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[p] = red[0];
}

// MODE 1: out = dout o sign(op . x)  (filtered slice)  |  dout o sign(x)  (other slices)
// MODE 2: out (+)= op . x             (filtered slice)  |  x               (other slices)
// The product is evp_highpass_kernel's (32x32 output tile per workgroup, 2x2 per thread, the same FMA order over k).
template <int MODE>
__global__ __launch_bounds__(256) void evp_hp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ op, const int* __restrict__ dmask,
                                                         const float* __restrict__ dout, float* __restrict__ out, int D, int H, int W, int accumulate) {
  __shared__ float sA[32][33], sX[32][33];
  const int s = blockIdx.z, d = s % D;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float* xs = x + (size_t)s * H * W;
  const float* gs = MODE == 1 ? dout + (size_t)s * H * W : nullptr;
  float* os = out + (size_t)s * H * W;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  const bool filt = dmask[d] != 0;
  if (filt) {
    for (int k0 = 0; k0 < H; k0 += 32) {
      for (int t = threadIdx.x; t < 32 * 32; t += 256) {
        const int r = t >> 5, c = t & 31;
        sA[r][c] = (i0 + r < H && k0 + c < H) ? op[(size_t)(i0 + r) * H + k0 + c] : 0.f;
        sX[r][c] = (k0 + r < H && j0 + c < W) ? xs[(size_t)(k0 + r) * W + j0 + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < 32; ++k) {
        const float a0 = sA[ty * 2][k], a1 = sA[ty * 2 + 1][k], b0 = sX[k][tx * 2], b1 = sX[k][tx * 2 + 1];
        acc[0][0] = __builtin_fmaf(a0, b0, acc[0][0]); acc[0][1] = __builtin_fmaf(a0, b1, acc[0][1]);
        acc[1][0] = __builtin_fmaf(a1, b0, acc[1][0]); acc[1][1] = __builtin_fmaf(a1, b1, acc[1][1]);
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = i0 + ty * 2 + a, j = j0 + tx * 2 + b;
      if (i >= H || j >= W) continue;
      const size_t e = (size_t)i * W + j;
      const float v = filt ? acc[a][b] : xs[e];
      if (MODE == 1) {
        os[e] = v > 0.f ? gs[e] : (v < 0.f ? -gs[e] : 0.f);
      } else {
        os[e] = accumulate ? os[e] + v : v;
      }
    }
}

}  // namespace gvk

extern "C" int gvk_unpatchify_f32(const float* dcols, float* out, const float* x, const float* x0, int B, int D, int H, int W, int pd, int ph, int pw,
                                  int nsum, float alpha, float beta, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(dcols && out && B > 0 && nsum > 0 && pd > 0 && ph > 0 && pw > 0, "gvk_unpatchify_f32: bad arguments");
  GVK_REQUIRE(x != nullptr || x0 == nullptr, "gvk_unpatchify_f32: x0 without x");
  GVK_REQUIRE(D % pd == 0 && H % ph == 0 && W % pw == 0 && pw % 4 == 0,
              "gvk_unpatchify_f32: volume %dx%dx%d not divisible by patch %dx%dx%d (pw must be a multiple of 4)", D, H, W, pd, ph, pw);
  GVK_REQUIRE((((uintptr_t)dcols | (uintptr_t)out | (uintptr_t)x | (uintptr_t)x0) & 15) == 0, "gvk_unpatchify_f32: pointers must be 16-byte aligned");
  const int64_t total = (int64_t)B * D * H * (W / 4);
  GVK_LAUNCH(unpatchify_kernel, dim3(grid_blocks(total, 4096)), dim3(256), 0, (hipStream_t)stream, dcols, out, x, x0, B, D, H, W, pd, ph, pw, nsum, alpha, beta);
  return check_launch("unpatchify_f32");
}

extern "C" int gvk_patch_reduce_f32(const float* vol, float* out, int B, int D, int H, int W, int pd, int ph, int pw, int absval, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(vol && out && B > 0 && pd > 0 && ph > 0 && pw > 0, "gvk_patch_reduce_f32: bad arguments");
  GVK_REQUIRE(D % pd == 0 && H % ph == 0 && W % pw == 0 && pw % 4 == 0,
              "gvk_patch_reduce_f32: volume %dx%dx%d not divisible by patch %dx%dx%d (pw must be a multiple of 4)", D, H, W, pd, ph, pw);
  GVK_REQUIRE((((uintptr_t)vol) & 15) == 0, "gvk_patch_reduce_f32: the volume must be 16-byte aligned");
  const int64_t np = (int64_t)B * (D / pd) * (H / ph) * (W / pw);
  GVK_REQUIRE(np < (1LL << 31), "gvk_patch_reduce_f32: too many patches");
  GVK_LAUNCH(patch_reduce_kernel, dim3((unsigned)np), dim3(256), 0, (hipStream_t)stream, vol, out, D, H, W, pd, ph, pw, absval);
  return check_launch("patch_reduce_f32");
}

extern "C" int gvk_evp_highpass_sign(const float* img, const float* hp, const int32_t* depth_mask, const float* dout, float* out, int B, int D, int H,
                                     int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(img && hp && depth_mask && dout && out && B > 0 && D > 0 && H > 0 && W > 0, "gvk_evp_highpass_sign: bad arguments");
  GVK_LAUNCH(evp_hp_bwd_kernel<1>, dim3((W + 31) / 32, (H + 31) / 32, B * D), dim3(256), 0, (hipStream_t)stream, img, hp, (const int*)depth_mask, dout,
             out, D, H, W, 0);
  return check_launch("evp_highpass_sign");
}

extern "C" int gvk_evp_highpass_linear(const float* x, const float* op, const int32_t* depth_mask, float* out, int accumulate, int B, int D, int H,
                                       int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && op && depth_mask && out && B > 0 && D > 0 && H > 0 && W > 0, "gvk_evp_highpass_linear: bad arguments");
  GVK_REQUIRE(x != out, "gvk_evp_highpass_linear: out must not alias x (the product reads whole columns of x)");
  GVK_LAUNCH(evp_hp_bwd_kernel<2>, dim3((W + 31) / 32, (H + 31) / 32, B * D), dim3(256), 0, (hipStream_t)stream, x, op, (const int*)depth_mask,
             nullptr, out, D, H, W, accumulate);
  return check_launch("evp_highpass_linear");
}
