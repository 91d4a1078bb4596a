// Attention maps for model explanations (gaviko_amd/explain.py), bf16 path, head dim 64.
// The reference exposes the probabilities of every global self-attention through its nn.Softmax module
// (vision_transformer.py:50,67); the flash kernels here never build P.  What an explanation needs of P is a weighted sum of its
// rows -- the pooled query's map, one row, or the relevance vector of attention rollout:
//     out[b][h][j] = sum_{q0 <= i < q1} w[b][i] * P[b][h][i][j],   P = exp2(q'_i . k_j - lse[b][h][i] * log2 e)
// recomputed from the forward's own buffers (qkv with the q block pre-scaled by scale * log2 e, lse natural log), exactly the way the
// backward recomputes P.
//   colsum: workgroup = 128 keys (4 waves x 32) of one (batch, head), sweeping the query rows [q0, q1) in staged tiles of 64.  The
//           score tile is computed with the KEY on the MFMA lane (the structure of attn_bwd_dkdv_kernel): a lane's 16 accumulator
//           registers hold 16 query rows of its key, so the weighted sum over queries is a chain of fp32 FMAs inside the lane and one
//           swap of the two half-waves at the end.  S' - lse * log2 e (and the mask of rows past q1) rides an augmented MFMA
//           (attention_common.hpp).  No atomics: fixed summation order, bitwise reproducible.
//   rollout step: r_out = 0.5 r_in + (0.5 / H) sum_h out[h], heads summed in order.  A separate kernel: fused into colsum, one
//           workgroup would own a key tile for all heads -- B * ceil(T / 128) = 36 workgroups at B = 4, T = 1033 on 256 CUs,
//           against 432 for the per-head form.
//   gradcolsum: the class-specific counterpart (gradient x attention; Chefer, Gur & Wolf 2021) --
//               out[b][h][j] = sum_{q0 <= i < q1} w[b][i] * P[b][h][i][j] * max(0, dP[b][h][i][j]),   dP = dO_i . v_j
//           with dO the backward sweep's gradient of the attention output (the engine's bf16 dctx).  The colsum kernel with a second
//           MFMA chain: the wave keeps its keys' V fragments next to the K fragments, a dO tile is staged beside the Q tile, and dP
//           accumulates in the layout of S', so the two meet register by register in fp32 (neither is rounded to bf16).
//   relevance step: r_out = r_in + (1 / H) sum_h out[h], heads summed in order.
#include "attention_common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

static constexpr int kMapQT = 64;      // query rows per staged tile (two 32-row sub-blocks)

__global__ __launch_bounds__(256, 2) void attn_colsum_kernel(const bf16* __restrict__ qkv, const float* __restrict__ lse,
                                                          const float* __restrict__ w, int ld_w, float* __restrict__ out, int T, int H,
                                                          int ld_qkv, int q0, int q1) {
  __shared__ __attribute__((aligned(16))) char sQ[kMapQT * 128];     // [64 rows][64 bf16], 16-B chunks swizzled by attn_swz
  __shared__ __attribute__((aligned(16))) float sL[kMapQT];
  __shared__ __attribute__((aligned(16))) float sW[kMapQT];
  const int nkb = (T + 127) / 128;
  int bh, kblk;
  xcd_group_block(blockIdx.x, nkb, gridDim.x / nkb, bh, kblk);        // all key blocks of a (batch, head) on one XCD: they read the same Q rows
  const int b = bh / H, head = bh - b * H, k0 = kblk * 128;
  const int lane = lane_id(), wave = wave_id();
  const int r31 = lane & 31, hh = lane >> 5;
  const int inner = H * 64;
  const bf16* qbase = qkv + (size_t)b * T * ld_qkv + head * 64;
  const float* lrow = lse + (size_t)bh * T;
  const float* wrow = w + (size_t)b * ld_w;
  const bool active = k0 + wave * 32 < T;          // a wave whose 32 keys all lie past the sequence only stages tiles

  // K fragments of this wave's 32 keys: B operands (col = key, k = d); keys past the sequence read the last key and are not stored
  const int key = k0 + wave * 32 + r31;
  const int keyc = min(key, T - 1);
  bf16x8 kf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const bf16x8*)(qbase + inner + (size_t)keyc * ld_qkv + 16 * ks + 8 * hh);

  // staging: thread t carries 16-B chunks t and t + 256 of the [64][128 B] Q tile; threads 0..63 the row's lse and weight.  Rows past
  // q1 read row min(row, T - 1) (finite), get weight 0 and are masked to P = 0 by the augmented MFMA.
  const int tid = threadIdx.x;
  u32x4 pq[2];
  float pl = 0.f, pw = 0.f;
  auto fetch = [&](int qt0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, row = idx >> 3, c = idx & 7;
      const int g = min(qt0 + row, T - 1);
      pq[u] = *(const u32x4*)(qbase + (size_t)g * ld_qkv + c * 8);
    }
    if (tid < kMapQT) {
      const int g = qt0 + tid;
      pl = lrow[min(g, T - 1)];
      pw = g < q1 ? wrow[g] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, row = idx >> 3, c = idx & 7;
      *(u32x4*)(sQ + row * 128 + ((c ^ attn_swz(row)) << 4)) = pq[u];
    }
    if (tid < kMapQT) {
      sL[tid] = pl;
      sW[tid] = pw;
    }
  };

  const bf16x8 sel_s = aug_sel_first(true, hh);      // [1, 1, 1, 1, 0...]: the query side carries -3e38 only in rows past q1
  float acc = 0.f;                                   // this lane's key: sum over the query rows of its half-wave
  const int ntile = (q1 - q0 + kMapQT - 1) / kMapQT;
  fetch(q0);
  for (int t = 0; t < ntile; ++t) {
    const int qt0 = q0 + t * kMapQT;
    __syncthreads();                                 // the previous tile is consumed
    store();
    __syncthreads();
    if (t + 1 < ntile) fetch(qt0 + kMapQT);          // next tile's loads in flight behind this tile's arithmetic
    if (active) {
#pragma unroll
      for (int sub = 0; sub < kMapQT / 32; ++sub) {
        const int row0 = qt0 + sub * 32;
        if (row0 >= q1) break;                       // wave-uniform
        const char* sq = sQ + sub * 32 * 128;        // (32 rows = a multiple of the swizzle period 16)
        const float l2 = sL[sub * 32 + r31] * 1.44269504088896340736f;
        const bf16x8 qaug = aug_const(l2, row0 + r31 >= q1, 0.f, hh);
        // S'[q][key] = Q'.K^T - lse * log2 e   (A = query rows, B = this wave's keys)
        f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qaug, sel_s, f32x16{}, 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int chunk = 2 * ks + hh;
          const bf16x8 qa = *(const bf16x8*)(sq + r31 * 128 + ((chunk ^ attn_swz(r31)) << 4));
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
        }
        // accumulator register r holds query row (r & 3) + 8 (r >> 2) + 4 hh of the sub-block: its weights are four float4 pieces
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 wv = *(const float4*)(sW + sub * 32 + 8 * g4 + 4 * hh);
          acc = __builtin_fmaf(wv.x, __builtin_amdgcn_exp2f(s[4 * g4 + 0]), acc);
          acc = __builtin_fmaf(wv.y, __builtin_amdgcn_exp2f(s[4 * g4 + 1]), acc);
          acc = __builtin_fmaf(wv.z, __builtin_amdgcn_exp2f(s[4 * g4 + 2]), acc);
          acc = __builtin_fmaf(wv.w, __builtin_amdgcn_exp2f(s[4 * g4 + 3]), acc);
        }
      }
    }
  }
  acc = half_sum(acc);                               // lanes l and l + 32 hold the two halves of key l's rows
  if (active && hh == 0 && key < T) out[(size_t)bh * T + key] = acc;
}

__global__ __launch_bounds__(256) void rollout_step_kernel(const float* r_in, const float* __restrict__ colsum, float* r_out, int B, int T, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, j = i - b * T;
  const float* c = colsum + (size_t)b * H * T + j;
  float s = 0.f;
  for (int h = 0; h < H; ++h) s += c[(size_t)h * T];
  const float r = r_in[i];                           // (r_out may alias r_in: every element is read before it is written, by one thread)
  r_out[i] = 0.5f * r + (0.5f / (float)H) * s;
}

__global__ __launch_bounds__(256, 2) void attn_gradcolsum_kernel(const bf16* __restrict__ qkv, const float* __restrict__ lse,
                                                              const bf16* __restrict__ dctx, int ld_dctx, const float* __restrict__ w, int ld_w,
                                                              float* __restrict__ out, int T, int H, int ld_qkv, int q0, int q1) {
  __shared__ __attribute__((aligned(16))) char sQ[kMapQT * 128];     // [64 rows][64 bf16], 16-B chunks swizzled by attn_swz
  __shared__ __attribute__((aligned(16))) char sD[kMapQT * 128];     // the same rows of dO, same layout
  __shared__ __attribute__((aligned(16))) float sL[kMapQT];
  __shared__ __attribute__((aligned(16))) float sW[kMapQT];
  const int nkb = (T + 127) / 128;
  int bh, kblk;
  xcd_group_block(blockIdx.x, nkb, gridDim.x / nkb, bh, kblk);        // all key blocks of a (batch, head) on one XCD: they read the same Q / dO rows
  const int b = bh / H, head = bh - b * H, k0 = kblk * 128;
  const int lane = lane_id(), wave = wave_id();
  const int r31 = lane & 31, hh = lane >> 5;
  const int inner = H * 64;
  const bf16* qbase = qkv + (size_t)b * T * ld_qkv + head * 64;
  const bf16* dbase = dctx + (size_t)b * T * ld_dctx + head * 64;
  const float* lrow = lse + (size_t)bh * T;
  const float* wrow = w + (size_t)b * ld_w;
  const bool active = k0 + wave * 32 < T;          // a wave whose 32 keys all lie past the sequence only stages tiles

  // K and V fragments of this wave's 32 keys: B operands (col = key, k = d); keys past the sequence read the last key and are not stored
  const int key = k0 + wave * 32 + r31;
  const int keyc = min(key, T - 1);
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kf[ks] = *(const bf16x8*)(qbase + inner + (size_t)keyc * ld_qkv + 16 * ks + 8 * hh);
    vf[ks] = *(const bf16x8*)(qbase + 2 * inner + (size_t)keyc * ld_qkv + 16 * ks + 8 * hh);
  }

  // staging: thread t carries 16-B chunks t and t + 256 of the [64][128 B] Q tile and of the dO tile; threads 0..63 the row's lse and
  // weight.  Rows past q1 read row min(row, T - 1) of both (finite), get weight 0 and are masked to P = 0 by the augmented MFMA, so
  // their finite dP contributes an exact 0.
  const int tid = threadIdx.x;
  u32x4 pq[2], pd[2];
  float pl = 0.f, pw = 0.f;
  auto fetch = [&](int qt0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, row = idx >> 3, c = idx & 7;
      const int g = min(qt0 + row, T - 1);
      pq[u] = *(const u32x4*)(qbase + (size_t)g * ld_qkv + c * 8);
      pd[u] = *(const u32x4*)(dbase + (size_t)g * ld_dctx + c * 8);
    }
    if (tid < kMapQT) {
      const int g = qt0 + tid;
      pl = lrow[min(g, T - 1)];
      pw = g < q1 ? wrow[g] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = u * 256 + tid, row = idx >> 3, c = idx & 7;
      *(u32x4*)(sQ + row * 128 + ((c ^ attn_swz(row)) << 4)) = pq[u];
      *(u32x4*)(sD + row * 128 + ((c ^ attn_swz(row)) << 4)) = pd[u];
    }
    if (tid < kMapQT) {
      sL[tid] = pl;
      sW[tid] = pw;
    }
  };

  const bf16x8 sel_s = aug_sel_first(true, hh);      // [1, 1, 1, 1, 0...]: the query side carries -3e38 only in rows past q1
  float acc = 0.f;                                   // this lane's key: sum over the query rows of its half-wave
  const int ntile = (q1 - q0 + kMapQT - 1) / kMapQT;
  fetch(q0);
  for (int t = 0; t < ntile; ++t) {
    const int qt0 = q0 + t * kMapQT;
    __syncthreads();                                 // the previous tile is consumed
    store();
    __syncthreads();
    if (t + 1 < ntile) fetch(qt0 + kMapQT);          // next tile's loads in flight behind this tile's arithmetic
    if (active) {
#pragma unroll
      for (int sub = 0; sub < kMapQT / 32; ++sub) {
        const int row0 = qt0 + sub * 32;
        if (row0 >= q1) break;                       // wave-uniform
        const char* sq = sQ + sub * 32 * 128;        // (32 rows = a multiple of the swizzle period 16)
        const char* sd = sD + sub * 32 * 128;
        const float l2 = sL[sub * 32 + r31] * 1.44269504088896340736f;
        const bf16x8 qaug = aug_const(l2, row0 + r31 >= q1, 0.f, hh);
        // S'[q][key] = Q'.K^T - lse * log2 e  and  dP[q][key] = dO.V^T   (A = query rows, B = this wave's keys): the same register of the
        // two accumulators is the same (query, key)
        f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qaug, sel_s, f32x16{}, 0, 0, 0);
        f32x16 dp = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int off = r31 * 128 + (((2 * ks + hh) ^ attn_swz(r31)) << 4);
          const bf16x8 qa = *(const bf16x8*)(sq + off);
          const bf16x8 da = *(const bf16x8*)(sd + off);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], dp, 0, 0, 0);
        }
        // accumulator register r holds query row (r & 3) + 8 (r >> 2) + 4 hh of the sub-block: its weights are four float4 pieces
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 wv = *(const float4*)(sW + sub * 32 + 8 * g4 + 4 * hh);
          acc = __builtin_fmaf(wv.x * __builtin_amdgcn_exp2f(s[4 * g4 + 0]), fmaxf(dp[4 * g4 + 0], 0.f), acc);
          acc = __builtin_fmaf(wv.y * __builtin_amdgcn_exp2f(s[4 * g4 + 1]), fmaxf(dp[4 * g4 + 1], 0.f), acc);
          acc = __builtin_fmaf(wv.z * __builtin_amdgcn_exp2f(s[4 * g4 + 2]), fmaxf(dp[4 * g4 + 2], 0.f), acc);
          acc = __builtin_fmaf(wv.w * __builtin_amdgcn_exp2f(s[4 * g4 + 3]), fmaxf(dp[4 * g4 + 3], 0.f), acc);
        }
      }
    }
  }
  acc = half_sum(acc);                               // lanes l and l + 32 hold the two halves of key l's rows
  if (active && hh == 0 && key < T) out[(size_t)bh * T + key] = acc;
}

__global__ __launch_bounds__(256) void relevance_step_kernel(const float* r_in, const float* __restrict__ colsum, float* r_out, int B, int T, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, j = i - b * T;
  const float* c = colsum + (size_t)b * H * T + j;
  float s = 0.f;
  for (int h = 0; h < H; ++h) s += c[(size_t)h * T];
  const float r = r_in[i];                           // (r_out may alias r_in: every element is read before it is written, by one thread)
  r_out[i] = r + (1.0f / (float)H) * s;
}

}  // namespace gvk

extern "C" int gvk_attention_colsum_bf16(const void* qkv, const float* lse, const float* w, int ld_w, float* out, int B, int T, int H, int ld_qkv,
                                         int q0, int q1, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(qkv && lse && w && out, "gvk_attention_colsum_bf16: null pointer");
  GVK_REQUIRE(B > 0 && T > 0 && H > 0, "gvk_attention_colsum_bf16: empty shape");
  GVK_REQUIRE(0 <= q0 && q0 < q1 && q1 <= T, "gvk_attention_colsum_bf16: query rows [%d, %d) outside [0, T = %d)", q0, q1, T);
  GVK_REQUIRE(ld_w >= T, "gvk_attention_colsum_bf16: ld_w=%d < T=%d", ld_w, T);
  GVK_REQUIRE(ld_qkv >= 3 * H * 64 && ld_qkv % 8 == 0, "gvk_attention_colsum_bf16: head dim is fixed at 64; ld_qkv=%d inconsistent with H=%d", ld_qkv, H);
  GVK_REQUIRE((int64_t)B * H * ((T + 127) / 128) < (int64_t)1 << 31, "gvk_attention_colsum_bf16: grid too large");
  const dim3 grid((unsigned)(B * H * ((T + 127) / 128)));
  GVK_LAUNCH(attn_colsum_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, lse, w, ld_w, out, T, H, ld_qkv, q0, q1);
  return check_launch("attention_colsum");
}

extern "C" int gvk_rollout_step(const float* r_in, const float* colsum, float* r_out, int B, int T, int H, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(r_in && colsum && r_out, "gvk_rollout_step: null pointer");
  GVK_REQUIRE(B > 0 && T > 0 && H > 0 && (int64_t)B * T < (int64_t)1 << 31, "gvk_rollout_step: bad shape");
  GVK_LAUNCH(rollout_step_kernel, dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r_in, colsum, r_out, B, T, H);
  return check_launch("rollout_step");
}

extern "C" int gvk_attention_gradcolsum_bf16(const void* qkv, const float* lse, const void* dctx, int ld_dctx, const float* w, int ld_w, float* out,
                                             int B, int T, int H, int ld_qkv, int q0, int q1, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(qkv && lse && dctx && w && out, "gvk_attention_gradcolsum_bf16: null pointer");
  GVK_REQUIRE(B > 0 && T > 0 && H > 0, "gvk_attention_gradcolsum_bf16: empty shape");
  GVK_REQUIRE(0 <= q0 && q0 < q1 && q1 <= T, "gvk_attention_gradcolsum_bf16: query rows [%d, %d) outside [0, T = %d)", q0, q1, T);
  GVK_REQUIRE(ld_w >= T, "gvk_attention_gradcolsum_bf16: ld_w=%d < T=%d", ld_w, T);
  GVK_REQUIRE(ld_qkv >= 3 * H * 64 && ld_qkv % 8 == 0, "gvk_attention_gradcolsum_bf16: head dim is fixed at 64; ld_qkv=%d inconsistent with H=%d", ld_qkv, H);
  GVK_REQUIRE(ld_dctx >= H * 64 && ld_dctx % 8 == 0, "gvk_attention_gradcolsum_bf16: ld_dctx=%d inconsistent with H=%d (head dim 64)", ld_dctx, H);
  GVK_REQUIRE((int64_t)B * H * ((T + 127) / 128) < (int64_t)1 << 31, "gvk_attention_gradcolsum_bf16: grid too large");
  const dim3 grid((unsigned)(B * H * ((T + 127) / 128)));
  GVK_LAUNCH(attn_gradcolsum_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, lse, (const bf16*)dctx, ld_dctx, w, ld_w, out, T, H,
             ld_qkv, q0, q1);
  return check_launch("attention_gradcolsum");
}

extern "C" int gvk_relevance_step(const float* r_in, const float* colsum, float* r_out, int B, int T, int H, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(r_in && colsum && r_out, "gvk_relevance_step: null pointer");
  GVK_REQUIRE(B > 0 && T > 0 && H > 0 && (int64_t)B * T < (int64_t)1 << 31, "gvk_relevance_step: bad shape");
  GVK_LAUNCH(relevance_step_kernel, dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r_in, colsum, r_out, B, T, H);
  return check_launch("relevance_step");
}
