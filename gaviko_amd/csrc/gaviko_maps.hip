// Probability maps of GAViKO's own attentions for explanations (gaviko_amd/explain.py): the masked-window local self-attention (MWSA,
// gaviko.py:235-238) and the two prompt cross-attentions of the gated prompt awakening (GPA, gaviko.py:84-94,175-178).  The training
// kernels (window_attn.hip, gpa.hip) never build a probability; both maps are recomputed from the buffers a forward leaves, against its
// own log-sum-exp, as the backward passes do.  fp32 throughout (the side paths are fp32 on both precision paths).
#include "common.hpp"
#include "cross.hpp"
#include "window_args.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

struct WinColsumArgs {
  const float* qkv;   // [B*N][3L]
  const float* lse;   // [B*N]
  const float* w;     // [B][N]
  float* out;         // [B][N]
  int B, D, H, W, kd, kh, kw;
  float scale;
};

// out[b][j] = sum_i w[b][i] P[b][i][j]: the key-side pass of the window backward (win_bwd_kv_kernel) with the scalar w_i in the place of
// dctx_i.  One wave per key j, lanes over the queries of its REVERSE window, partial sums folded by a butterfly: no atomics, fixed order.
template <int L>
__global__ __launch_bounds__(256) void win_colsum_kernel(WinColsumArgs p) {
  const int N = p.D * p.H * p.W;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B * N) return;
  const int lane = lane_id();
  const int b = row / N, j = row - b * N;
  const int kd_ = j / (p.H * p.W), kh_ = (j / p.W) % p.H, kw_ = j % p.W;
  Win w;
  axis_rev(kd_, p.kd, p.D, w.d0, w.nd);
  axis_rev(kh_, p.kh, p.H, w.h0, w.nh);
  axis_rev(kw_, p.kw, p.W, w.w0, w.nw);
  const int nq = w.count();
  const float* base = p.qkv + (size_t)b * N * 3 * L;
  float k[L];
#pragma unroll
  for (int l = 0; l < L; ++l) k[l] = base[(size_t)j * 3 * L + L + l];
  float acc = 0.f;
  for (int qq = lane; qq < nq; qq += 64) {
    const int i = w.index(qq, p.H, p.W);
    const size_t gi = (size_t)b * N + i;
    const float wi = p.w[gi];
    const float* qr = base + (size_t)i * 3 * L;
    float d = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) d += (qr[l] * p.scale) * k[l];            // the forward's own rounding: q is scaled first (win_fwd_kernel)
    acc = __builtin_fmaf(wi, __expf(d - p.lse[gi]), acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) p.out[row] = acc;
}

struct GpaMapsArgs {
  const float* xl; const float* ll;          // [B*T][L], [B*N][L]
  const float* qg; const float* ql;          // [B][P][L], pre-scaled by L^-1/2 (gpa_fwd_kernel)
  const float* lse_g; const float* lse_l;    // [B][P], natural log
  const float* imp; const float* gw;         // [B][P], [B]
  float* pg; float* pl; float* fused;        // [B][P][N], each may be NULL
  int B, T, N, P;
};

// One lane per patch position n: its local latent and its global latent are read once (contiguous rows: consecutive lanes read consecutive
// 4L-byte rows) and meet all P queries of the sample, which sit in LDS with their statistics; every store is a run of consecutive n.
// Global side: the reference slices the image tokens twice (gaviko.py:161,107), so the softmax runs over global rows 2P+2 .. T-1 only --
// patch positions n >= P+1 (row P+1+n of xl); the first P+1 positions carry probability 0.
template <int L>
__global__ __launch_bounds__(256) void gpa_maps_kernel(GpaMapsArgs p) {
  __shared__ float qg_s[64 * L], ql_s[64 * L], lg_s[64], ll_s[64], im_s[64];
  const int b = blockIdx.y, P = p.P;
  for (int i = threadIdx.x; i < P * L; i += 256) {
    qg_s[i] = p.qg[(size_t)b * P * L + i];
    ql_s[i] = p.ql[(size_t)b * P * L + i];
  }
  for (int i = threadIdx.x; i < P; i += 256) {
    lg_s[i] = p.lse_g[b * P + i]; ll_s[i] = p.lse_l[b * P + i]; im_s[i] = p.imp[b * P + i];
  }
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= p.N) return;
  const float gw = p.gw[b];
  const bool has_g = n >= P + 1;                                           // (P + 1 + n <= T - 1 = P + N: inside xl)
  float tg[L], tl[L];
  load_tok<L>(p.ll + (size_t)b * p.N * L, n, p.N, tl);
  load_tok<L>(p.xl + ((size_t)b * p.T + P + 1) * L, n, p.N, tg);
  for (int q = 0; q < P; ++q) {
    float dg = 0.f, dl = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      dg = __builtin_fmaf(qg_s[q * L + l], tg[l], dg);
      dl = __builtin_fmaf(ql_s[q * L + l], tl[l], dl);
    }
    const float ag = has_g ? __expf(dg - lg_s[q]) : 0.f;
    const float al = __expf(dl - ll_s[q]);
    const size_t o = ((size_t)b * P + q) * p.N + n;
    if (p.pg) p.pg[o] = ag;
    if (p.pl) p.pl[o] = al;
    if (p.fused) p.fused[o] = im_s[q] * (gw * ag + (1.f - gw) * al);
  }
}

}  // namespace gvk

extern "C" int gvk_window_attn_colsum(const gvk_window_colsum_desc* d, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(d && d->qkv && d->lse && d->w && d->out, "gvk_window_attn_colsum: null pointer");
  GVK_REQUIRE(d->B > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->kd > 0 && d->kh > 0 && d->kw > 0, "gvk_window_attn_colsum: bad grid/window");
  GVK_REQUIRE((int64_t)d->B * d->D * d->H * d->W < (int64_t)1 << 31, "gvk_window_attn_colsum: grid too large");
  WinColsumArgs a{d->qkv, d->lse, d->w, d->out, d->B, d->D, d->H, d->W, d->kd, d->kh, d->kw, d->scale};
  hipStream_t s = (hipStream_t)stream;
  const int grid = (d->B * d->D * d->H * d->W + 3) / 4;
  switch (d->L) {
    case 4: GVK_LAUNCH((win_colsum_kernel<4>), dim3(grid), dim3(256), 0, s, a); break;
    case 8: GVK_LAUNCH((win_colsum_kernel<8>), dim3(grid), dim3(256), 0, s, a); break;
    case 16: GVK_LAUNCH((win_colsum_kernel<16>), dim3(grid), dim3(256), 0, s, a); break;
    case 20: GVK_LAUNCH((win_colsum_kernel<20>), dim3(grid), dim3(256), 0, s, a); break;
    case 32: GVK_LAUNCH((win_colsum_kernel<32>), dim3(grid), dim3(256), 0, s, a); break;
    default: return set_error(-2, "gvk_window_attn_colsum: L=%d unsupported (4, 8, 16, 20, 32)", d->L);
  }
  return check_launch("window_attn_colsum");
}

extern "C" int gvk_gpa_attn_maps(const gvk_gpa_maps_desc* d, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(d && d->xl && d->ll && d->qg && d->ql && d->lse_g && d->lse_l && d->imp && d->gw, "gvk_gpa_attn_maps: null input");
  GVK_REQUIRE(d->pg || d->pl || d->fused, "gvk_gpa_attn_maps: no output");
  GVK_REQUIRE(d->B > 0 && d->B <= 65535 && d->P > 0 && d->P <= 64 && d->N > 0, "gvk_gpa_attn_maps: need 0 < P <= 64, 0 < B <= 65535 (P=%d, B=%d)", d->P, d->B);
  GVK_REQUIRE(d->T == d->P + 1 + d->N, "gvk_gpa_attn_maps: T=%d is not P + 1 + N = %d (rows [prompts | cls | patches])", d->T, d->P + 1 + d->N);
  GVK_REQUIRE(d->N > d->P + 1, "gvk_gpa_attn_maps: N=%d leaves no global image tokens after the double slice (P=%d)", d->N, d->P);
  GpaMapsArgs a{d->xl, d->ll, d->qg, d->ql, d->lse_g, d->lse_l, d->imp, d->gw, d->pg, d->pl, d->fused, d->B, d->T, d->N, d->P};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((d->N + 255) / 256, d->B);
  switch (d->L) {
    case 4: GVK_LAUNCH((gpa_maps_kernel<4>), grid, dim3(256), 0, s, a); break;
    case 8: GVK_LAUNCH((gpa_maps_kernel<8>), grid, dim3(256), 0, s, a); break;
    case 16: GVK_LAUNCH((gpa_maps_kernel<16>), grid, dim3(256), 0, s, a); break;
    case 20: GVK_LAUNCH((gpa_maps_kernel<20>), grid, dim3(256), 0, s, a); break;
    case 32: GVK_LAUNCH((gpa_maps_kernel<32>), grid, dim3(256), 0, s, a); break;
    default: return set_error(-2, "gvk_gpa_attn_maps: L=%d unsupported (4, 8, 16, 20, 32)", d->L);
  }
  return check_launch("gpa_attn_maps");
}
