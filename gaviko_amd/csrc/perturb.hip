// Perturbation of the input volume at patch granularity (occlusion sensitivity, deletion / insertion curves): many inference forwards of
// one volume in which a chosen set of patches is replaced by a baseline.
//   patch_rank      relevance row -> position of every patch in the stable descending order (the inverse of a stable argsort).
//   patch_mask_*    per output sample a uint8 patch mask, from a rank interval [lo, hi) or from a box in patch-grid coordinates; the
//                   per-sample tables live in device memory, so a sweep uploads them once and every chunk reads its own slice.
//   perturb_volume  the HBM pass: out[o][v] = mask[o][patch(v)] ? fill : x[src[o]][v], written straight into the engine's input slot.
//                   The voxel <-> patch index map is patchify_kernel's (elementwise.hip) / unpatchify_kernel's (input_grad.hip).
//   perturb_scores  logits -> softmax probability and logit of the explained class, at device-resident output slots.
//   curve_auc       trapezoid area of a finished curve over x = k / N.
#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// rank[s][n] = #{m : rel[s][m] > rel[s][n]} + #{m < n : rel[s][m] == rel[s][n]}.  One workgroup per row, the row in LDS; every thread
// walks the whole row for each of its elements (all lanes read the same LDS word: a broadcast).  N^2 compares, no atomics: deterministic.
__global__ __launch_bounds__(256) void patch_rank_kernel(const float* __restrict__ rel, int* __restrict__ rank, int N) {
  extern __shared__ float row[];
  const float* r = rel + (int64_t)blockIdx.x * N;
  for (int i = threadIdx.x; i < N; i += 256) row[i] = r[i];
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += 256) {
    const float v = row[n];
    int c = 0;
    for (int m = 0; m < N; ++m) {
      const float u = row[m];
      c += (u > v || (u == v && m < n)) ? 1 : 0;
    }
    rank[(int64_t)blockIdx.x * N + n] = c;
  }
}

// mask[o][n] = lo[o] <= rank[src[o]][n] < hi[o].  The table values are the caller's contract (gaviko_amd.explain builds them itself); a source
// index outside [0, S) masks nothing rather than reading outside rank.
__global__ __launch_bounds__(256) void patch_mask_rank_kernel(const int* __restrict__ rank, const int* __restrict__ src, const int* __restrict__ lo,
                                                              const int* __restrict__ hi, uint8_t* __restrict__ mask, int Bout, int S, int N) {
  const int64_t total = (int64_t)Bout * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i / N), n = (int)(i - (int64_t)o * N);
    const int s = src[o];
    uint8_t m = 0;
    if (s >= 0 && s < S) {
      const int r = rank[(int64_t)s * N + n];
      m = (r >= lo[o] && r < hi[o]) ? 1 : 0;
    }
    mask[i] = m;
  }
}

// mask[o][(d, h, w)] = the patch lies in box[o] = [d0, d1) x [h0, h1) x [w0, w1) (patch-grid units; a box that sticks out is clipped by
// the grid itself).
__global__ __launch_bounds__(256) void patch_mask_box_kernel(const int* __restrict__ boxes, uint8_t* __restrict__ mask, int Bout, int nd, int nh, int nw) {
  const int N = nd * nh * nw;
  const int64_t total = (int64_t)Bout * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i / N), n = (int)(i - (int64_t)o * N);
    const int w = n % nw, h = (n / nw) % nh, d = n / (nw * nh);
    const int* b = boxes + (int64_t)o * 6;
    mask[i] = (d >= b[0] && d < b[1] && h >= b[2] && h < b[3] && w >= b[4] && w < b[5]) ? 1 : 0;
  }
}

// out[o][v] = mask[o][patch(v)] ? (fill != nullptr ? fill[src[o]] : base[(nbase == 1 ? 0 : src[o])][v]) : x[src[o]][v].
// A selection of 32-bit words, no arithmetic: the output carries the bits of its source (signed zeros, denormals, NaN payloads).
// VEC = 4: one thread per 4 consecutive voxels along W (pw % 4 == 0, so they lie in one patch), 16-byte loads and stores.  VEC = 1: one
// thread per voxel, any geometry.
// Algorithmic bytes per launch: Bout * V * 4 written, at most (S + nbase) * V * 4 read from HBM (every source volume once; the outputs that
// share a source re-read it from cache), plus the Bout * N mask bytes.
template <int VEC>
__global__ __launch_bounds__(256) void perturb_volume_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ mask, const int* __restrict__ src,
                                                             const uint32_t* __restrict__ fill, const uint32_t* __restrict__ base, int nbase,
                                                             uint32_t* __restrict__ out, int Bout, int S, int D, int H, int W, int pd, int ph, int pw) {
  // 32-bit index arithmetic: the entry point checks that Bout * D * H * (W / VEC) fits (64-bit divisions are emulated and sat in this loop)
  const unsigned nh = H / ph, nw = W / pw, uH = H, uD = D, upd = pd, uph = ph, upw = pw;
  const unsigned N = (D / pd) * nh * nw;
  const unsigned wq = W / VEC;
  const int64_t V = (int64_t)D * H * W;
  const unsigned total = (unsigned)Bout * uD * uH * wq;
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const unsigned row = idx / wq, xq = idx - row * wq;         // row = (o * D + z) * H + y
    const unsigned oz = row / uH, y = row - oz * uH;
    const unsigned o = oz / uD, z = oz - o * uD;
    const unsigned xx = xq * VEC;
    const unsigned n = ((z / upd) * nh + y / uph) * nw + xx / upw;
    const int64_t v = (int64_t)(z * uH + y) * W + xx;
    int s = src[o];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);                       // the values are the caller's contract; clamped so that nothing outside x is read
    const bool m = mask[(int64_t)o * N + n] != 0;
    if (VEC == 4) {
      u32x4 r;
      if (!m) {
        r = *(const u32x4*)(x + (int64_t)s * V + v);
      } else if (fill != nullptr) {
        const uint32_t f = fill[s];
        r = u32x4{f, f, f, f};
      } else {
        r = *(const u32x4*)(base + (nbase == 1 ? 0 : (int64_t)s * V) + v);
      }
      *(u32x4*)(out + (int64_t)o * V + v) = r;
    } else {
      uint32_t r;
      if (!m) r = x[(int64_t)s * V + v];
      else if (fill != nullptr) r = fill[s];
      else r = base[(nbase == 1 ? 0 : (int64_t)s * V) + v];
      out[(int64_t)o * V + v] = r;
    }
  }
}

// One workgroup per output sample o: p = softmax(logits[o])[target[src[o]]] (max-subtracted, fp32), written with the logit itself (and,
// if asked, the whole logits row) at slot slot[o]; slot[o] < 0 (the padding of a last chunk) writes nothing.  prob == nullptr: the rows
// only (a sweep gathers every chunk's logits and scores them in one launch at its end).  Every thread reduces a fixed strided subset in
// order, then a fixed tree in LDS: deterministic.  src and target values are the caller's contract; they are clamped into range, never trusted.
__global__ __launch_bounds__(256) void perturb_scores_kernel(const float* __restrict__ logits, const int* __restrict__ src, const int* __restrict__ target,
                                                             const int* __restrict__ slot, float* __restrict__ prob, float* __restrict__ logit,
                                                             float* __restrict__ rows, int S, int K, int nslots) {
  __shared__ float red[256];
  const int o = blockIdx.x;
  const int sl = slot[o];
  if (sl < 0 || sl >= nslots) return;                           // uniform over the workgroup
  const float* z = logits + (int64_t)o * K;
  if (rows != nullptr)
    for (int k = threadIdx.x; k < K; k += 256) rows[(int64_t)sl * K + k] = z[k];
  if (prob == nullptr) return;                                  // gather only (uniform)
  int s = src[o];
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  int tg = target[s];
  tg = tg < 0 ? 0 : (tg >= K ? K - 1 : tg);
  float mx = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) mx = fmaxf(mx, z[k]);
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) sum += expf(z[k] - mx);
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    prob[sl] = expf(z[tg] - mx) / red[0];
    logit[sl] = z[tg];
  }
}

// auc[s] = sum_i (ks[i + 1] - ks[i]) / N * (prob[s][i] + prob[s][i + 1]) / 2, one thread per curve, summed in i order in double.
__global__ __launch_bounds__(64) void curve_auc_kernel(const float* __restrict__ prob, const int* __restrict__ ks, float* __restrict__ auc, int S, int P,
                                                       int N) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const float* p = prob + (int64_t)s * P;
  double a = 0.0;
  for (int i = 0; i + 1 < P; ++i) a += (double)(ks[i + 1] - ks[i]) * 0.5 * ((double)p[i] + (double)p[i + 1]);
  auc[s] = (float)(a / (double)N);
}

}  // namespace gvk

extern "C" int gvk_patch_rank(const float* rel, int32_t* rank, int S, int N, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(rel && rank && S > 0 && N > 0, "gvk_patch_rank: bad arguments");
  GVK_REQUIRE(N <= 16384, "gvk_patch_rank: N = %d patches exceed the 16384 one workgroup keeps in LDS", N);
  GVK_LAUNCH(patch_rank_kernel, dim3((unsigned)S), dim3(256), (unsigned)(N * sizeof(float)), (hipStream_t)stream, rel, (int*)rank, N);
  return check_launch("patch_rank");
}

extern "C" int gvk_patch_mask_rank(const int32_t* rank, const int32_t* src, const int32_t* lo, const int32_t* hi, uint8_t* mask, int Bout, int S, int N,
                                   void* stream) {
  using namespace gvk;
  GVK_REQUIRE(rank && src && lo && hi && mask && Bout > 0 && S > 0 && N > 0, "gvk_patch_mask_rank: bad arguments");
  GVK_LAUNCH(patch_mask_rank_kernel, dim3(grid_blocks((int64_t)Bout * N, 8192)), dim3(256), 0, (hipStream_t)stream, (const int*)rank, (const int*)src,
             (const int*)lo, (const int*)hi, mask, Bout, S, N);
  return check_launch("patch_mask_rank");
}

extern "C" int gvk_patch_mask_box(const int32_t* boxes, uint8_t* mask, int Bout, int nd, int nh, int nw, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(boxes && mask && Bout > 0 && nd > 0 && nh > 0 && nw > 0, "gvk_patch_mask_box: bad arguments");
  GVK_REQUIRE((int64_t)nd * nh * nw < (1LL << 24), "gvk_patch_mask_box: patch grid %dx%dx%d too large", nd, nh, nw);
  GVK_LAUNCH(patch_mask_box_kernel, dim3(grid_blocks((int64_t)Bout * nd * nh * nw, 8192)), dim3(256), 0, (hipStream_t)stream, (const int*)boxes, mask, Bout,
             nd, nh, nw);
  return check_launch("patch_mask_box");
}

extern "C" int gvk_perturb_volume(const float* x, const uint8_t* mask, const int32_t* src, const float* fill_scalar, const float* base, int nbase,
                                  float* out, int Bout, int S, int D, int H, int W, int pd, int ph, int pw, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && mask && src && out && Bout > 0 && S > 0 && pd > 0 && ph > 0 && pw > 0, "gvk_perturb_volume: bad arguments");
  GVK_REQUIRE((fill_scalar != nullptr) != (base != nullptr), "gvk_perturb_volume: exactly one of fill_scalar and base");
  GVK_REQUIRE(base == nullptr || nbase == 1 || nbase == S, "gvk_perturb_volume: %d baseline volumes for %d sources (1 or one each)", nbase, S);
  GVK_REQUIRE(D > 0 && H > 0 && W > 0 && D % pd == 0 && H % ph == 0 && W % pw == 0, "gvk_perturb_volume: volume %dx%dx%d not divisible by patch %dx%dx%d",
              D, H, W, pd, ph, pw);
  const int64_t V = (int64_t)D * H * W;
  GVK_REQUIRE(out + (int64_t)Bout * V <= x || x + (int64_t)S * V <= out, "gvk_perturb_volume: out must not overlap x");
  GVK_REQUIRE(base == nullptr || out + (int64_t)Bout * V <= base || base + (int64_t)nbase * V <= out, "gvk_perturb_volume: out must not overlap base");
  GVK_REQUIRE((int64_t)Bout * V < (1LL << 31), "gvk_perturb_volume: %d x %lld voxels per launch exceed the 32-bit index range", Bout, (long long)V);
  const bool vec = pw % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)base) & 15) == 0;
  const uint32_t *xb = (const uint32_t*)x, *fb = (const uint32_t*)fill_scalar, *bb = (const uint32_t*)base;
  if (vec)
    GVK_LAUNCH(perturb_volume_kernel<4>, dim3(grid_blocks((int64_t)Bout * V / 4, 8192)), dim3(256), 0, (hipStream_t)stream, xb, mask, (const int*)src, fb, bb,
               nbase, (uint32_t*)out, Bout, S, D, H, W, pd, ph, pw);
  else
    GVK_LAUNCH(perturb_volume_kernel<1>, dim3(grid_blocks((int64_t)Bout * V, 8192)), dim3(256), 0, (hipStream_t)stream, xb, mask, (const int*)src, fb, bb, nbase,
               (uint32_t*)out, Bout, S, D, H, W, pd, ph, pw);
  return check_launch("perturb_volume");
}

extern "C" int gvk_perturb_scores(const float* logits, const int32_t* src, const int32_t* target, const int32_t* slot, float* prob, float* logit,
                                  float* rows, int Bout, int S, int K, int nslots, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(logits && slot && Bout > 0 && K > 0 && nslots > 0, "gvk_perturb_scores: bad arguments");
  GVK_REQUIRE(prob != nullptr || rows != nullptr, "gvk_perturb_scores: nothing to write (neither prob / logit nor rows)");
  GVK_REQUIRE(prob == nullptr ? logit == nullptr : (logit && src && target && S > 0), "gvk_perturb_scores: prob, logit, src and target go together");
  GVK_REQUIRE(rows == nullptr || rows + (int64_t)nslots * K <= logits || logits + (int64_t)Bout * K <= rows, "gvk_perturb_scores: rows must not overlap logits");
  GVK_LAUNCH(perturb_scores_kernel, dim3((unsigned)Bout), dim3(256), 0, (hipStream_t)stream, logits, (const int*)src, (const int*)target,
             (const int*)slot, prob, logit, rows, S, K, nslots);
  return check_launch("perturb_scores");
}

extern "C" int gvk_curve_auc(const float* prob, const int32_t* ks, float* auc, int S, int P, int N, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(prob && ks && auc && S > 0 && P > 0 && N > 0, "gvk_curve_auc: bad arguments");
  GVK_LAUNCH(curve_auc_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, (hipStream_t)stream, prob, (const int*)ks, auc, S, P, N);
  return check_launch("curve_auc");
}
