// The rest of torchio's MRI augmentation family on the device: tio.RandomGhosting, tio.RandomSpike, tio.RandomGamma, tio.RandomAnisotropy
// on a batch of fp32 volumes [B][D][H][W] already in HBM.  Three kernels, every one with per-sample DEVICE tables so that one launch serves
// a batch in which each sample drew something different, or nothing; no atomics anywhere: the same bits on every run.
//
// gvk_axis_circular_conv (ghosting).  torchio scales every n-th plane of the shifted spectrum along ONE axis and keeps the centre plane.  The
// mask does not depend on the other two frequency axes, so their transforms cancel against the inverses, exactly as in motion.hip; what is
// left is a real circular convolution along that axis,  y[..i..] = sum_i' c[(i - i') mod N] x[..i'..],  with the row c built on the host in
// float64 (data.ghosting_tables).  Unlike RandomMotion the axis is drawn per sample and can be any of the three:
//   axis 2  Y = X . C,  X = 32 (d, h) lines of W voxels (circulant.hpp);
//   axis 0  Y = C . X,  X = [D x 32 columns of the flattened H*W axis], rows H*W apart;
//   axis 1  Y = C . X,  X = [H x 32 columns of W] of one d, rows W apart.
// In the two left-multiply forms the contraction axis is the strided one and the columns are contiguous, so every global access still runs
// along W (32 voxels = one 128-byte line per row and instruction half).  The circulant is never materialised: every lane reads its element
// c[(i - i') mod N] from a doubled copy of the row in LDS.  The product runs on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: fp32
// operands, one rounding per product, fp32 accumulation in k order = an fmaf chain); bf16 operands would not do, for the reason at the top of
// motion.hip: c is an impulse minus small terms, on raw intensities of ~1e3.  Every output element is written once.
//
// gvk_gamma_spike: one streaming pass.  Gamma is sign(x) |x|^gamma; a spike in k-space is one complex exponential in image space, whose real
// part is kept: a cosine of a sum of three per-axis phases.  The phases are reduced modulo N in integers on the host, tabulated per axis as
// cos / sin in float64 (data.spike_tables) and combined here with the angle-addition formulas, so no large argument ever reaches a float.
//
// gvk_axis_gather2 (anisotropy): nearest-neighbour downsampling along one axis followed by linear upsampling collapses to two taps per output
// index; the host does all coordinate arithmetic in float64 (data.anisotropy_tables) and the device only gathers and blends.
#include "circulant.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kAcMaxN = GVK_AXIS_CONV_MAX_N;
constexpr int kAcLines = 32;                                   // axis 2: lines per workgroup, two 16-row tiles, one per wave parity
constexpr int kAcCols = 32;                                    // axes 0, 1: columns per workgroup, two 16-column tiles, one per wave parity
constexpr int kAcTiles = kAcMaxN / 32;                         // 16-wide tiles of the convolved axis one wave owns at most
static_assert(kAcMaxN == 256 && kAcMaxN % 32 == 0, "the tile lists and strides below assume a cap of 256");

// LDS strides, by the bank rule stated at circulant_stride, which is the stride of axis 2.
// Axes 0 and 1, B operand = x[k = l >> 4][column l & 15]: bank = stride * k + column, so the stride is 16 above a multiple of 32.
constexpr int kAcColStride = kAcCols + 16;
constexpr int kAcLdsX = kAcMaxN * kAcColStride > kAcLines * circulant_stride(kAcMaxN) ? kAcMaxN * kAcColStride : kAcLines * circulant_stride(kAcMaxN);

// 256 threads = 4 waves.  One grid serves the three forms: blockIdx.y = sample, blockIdx.x = work item of that sample's form (the grid is
// sized for the form with the most items; the others' surplus workgroups leave at once).  The waves split the tiles as circulant.hpp says,
// in the left-multiply forms with v & 1 choosing 16 of the 32 columns; nt = ceil(tiles / 2) <= 8 accumulators are live, and the fully
// unrolled loops skip the others with a wave-uniform test.
__global__ __launch_bounds__(256) void axis_circular_conv_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ ctab,
                                                                 const int* __restrict__ axis, const int* __restrict__ live, int D, int H, int W) {
  __shared__ float s_x[kAcLdsX];                               // the operand slab, then the output tile
  __shared__ float s_c[2 * kAcMaxN + 16];                      // s_c[i] = c[(i - Nk) mod N]: the circulant at offset (row - k) + Nk
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int DH = D * H, HW = H * W;
  const size_t V = (size_t)DH * W;
  const float* src = in + (size_t)b * V;
  float* dst = out + (size_t)b * V;
  const int ax = __builtin_amdgcn_readfirstlane(axis[b]);
  if (!live[b] || ax < 0 || ax > 2) {                          // block-uniform: this sample drew nothing, its bits pass through
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < V; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    return;
  }
  const int N = ax == 0 ? D : ax == 1 ? H : W;                 // extent of the convolved axis
  const int wchunks = (W + kAcCols - 1) / kAcCols;
  const int nwork = ax == 2 ? (DH + kAcLines - 1) / kAcLines : ax == 1 ? D * wchunks : (HW + kAcCols - 1) / kAcCols;
  if ((int)blockIdx.x >= nwork) return;
  const int Nk = (N + 15) & ~15, N4 = (N + 3) & ~3;            // rows / columns of the output tiles; k extent of the product (k = N.. are zero)
  const int ntile = Nk >> 4, nt = (ntile + 1) >> 1;
  circulant_fill_row(s_c, ctab + (size_t)b * kAcMaxN, N, Nk, tid);
  f32x4 acc[kAcTiles];
#pragma unroll
  for (int i = 0; i < kAcTiles; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int half = wave & 1, t0 = wave >> 1;

  if (ax == 2) {                                               // Y = X . C: 32 lines, contraction along the contiguous axis
    const int line0 = blockIdx.x * kAcLines;
    const int nlines = min(kAcLines, DH - line0);
    const int S = circulant_stride(Nk);
    for (int r = wave; r < kAcLines; r += 4)                   // a wave per line, lanes along W: coalesced; lines past the volume and columns
      for (int w = lane; w < S; w += 64)                       // past W are zero and contribute nothing
        s_x[r * S + w] = (r < nlines && w < W) ? src[(size_t)(line0 + r) * W + w] : 0.f;
    __syncthreads();
    circulant_product<kAcTiles>(acc, nt, s_x, S, s_c, Nk, N4, half, t0, lane);
    circulant_store_lines<kAcTiles>(acc, nt, s_x, S, dst, line0, nlines, W, Nk, half, t0, wave, lane);
    return;
  }

  // Y = C . X: N rows `rs` voxels apart, 32 contiguous columns of them
  size_t base;
  int rs, ncols;
  if (ax == 0) {
    const int col0 = blockIdx.x * kAcCols;
    base = (size_t)col0, rs = HW, ncols = min(kAcCols, HW - col0);
  } else {
    const int d = blockIdx.x / wchunks, w0 = (blockIdx.x - d * wchunks) * kAcCols;
    base = (size_t)d * HW + w0, rs = W, ncols = min(kAcCols, W - w0);
  }
  for (int r = tid >> 5; r < N4; r += 8)                       // half a wave per row, lanes along W; rows N.. and columns past the slab are zero
    s_x[r * kAcColStride + (tid & 31)] = (r < N && (tid & 31) < ncols) ? src[base + (size_t)r * rs + (tid & 31)] : 0.f;
  __syncthreads();
  // lane l holds A[row l & 15][k = k0 + (l >> 4)] = c[(row - k) mod N] and B[k = k0 + (l >> 4)][column l & 15]
  const float* ca = s_c + t0 * 16 + (lane & 15) - (lane >> 4) + Nk;
  const float* xb = s_x + (lane >> 4) * kAcColStride + half * 16 + (lane & 15);
  for (int k0 = 0; k0 < N4; k0 += 4) {
    const float bv = xb[k0 * kAcColStride];
#pragma unroll
    for (int i = 0; i < kAcTiles; ++i)
      if (i < nt) acc[i] = mfma4(ca[i * 32 - k0], bv, acc[i]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kAcTiles; ++i) {
    const int rt = t0 + 2 * i;
    if (i < nt && rt < ntile)                                  // wave-uniform
#pragma unroll
      for (int e = 0; e < 4; ++e) s_x[(rt * 16 + (lane >> 4) * 4 + e) * kAcColStride + half * 16 + (lane & 15)] = acc[i][e];
  }
  __syncthreads();
  for (int r = tid >> 5; r < N; r += 8)
    if ((tid & 31) < ncols) dst[base + (size_t)r * rs + (tid & 31)] = s_x[r * kAcColStride + (tid & 31)];
}

// ---- gamma and spikes -------------------------------------------------------------------------------------------------------------------
constexpr int kGsChunk = 4096;                                 // voxels per workgroup: 16 per thread, lanes along W
constexpr int kStatWords = GVK_NORMALIZE_STATS;

__global__ __launch_bounds__(256) void gamma_spike_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ kind,
                                                          const float* __restrict__ gamma, const float* __restrict__ amp,
                                                          const int* __restrict__ nspikes, const float* __restrict__ tab,
                                                          const double* __restrict__ stats, int D, int H, int W) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int HW = H * W, L = D + H + W;
  const size_t V = (size_t)D * HW;
  const float* src = in + (size_t)b * V;
  float* dst = out + (size_t)b * V;
  const size_t i0 = (size_t)blockIdx.x * kGsChunk;
  const int n = (int)min((size_t)kGsChunk, V - i0);
  const int k = __builtin_amdgcn_readfirstlane(kind[b]);
  if (k == GVK_KSPACE_GAMMA && gamma[b] != 1.0f) {             // gamma == 1 is the copy below: exactly the identity
    const float g = gamma[b];
    for (int i = tid; i < n; i += 256) {
      const float x = src[i0 + i];
      dst[i0 + i] = copysignf(powf(fabsf(x), g), x);
    }
  } else if (k == GVK_KSPACE_SPIKE) {
    const float scale = (float)((double)amp[b] * fabs(stats[(size_t)b * kStatWords + 2]));
    const int S = min(max(nspikes[b], 0), (int)GVK_SPIKE_MAX);
    const float* t = tab + (size_t)b * GVK_SPIKE_MAX * 2 * L;
    for (int i = tid; i < n; i += 256) {
      const size_t v = i0 + i;
      const int d = (int)(v / HW), r = (int)(v - (size_t)d * HW), h = r / W, w = r - h * W;
      float sum = 0.f;
      for (int s = 0; s < S; ++s) {
        const float* cs = t + (size_t)s * 2 * L;
        const float* sn = cs + L;
        const float c0 = cs[d], s0 = sn[d], c1 = cs[D + h], s1 = sn[D + h], c2 = cs[D + H + w], s2 = sn[D + H + w];
        const float p = c1 * c2 - s1 * s2;                     // cos(b1 + b2); nothing is contracted (the library builds with -ffp-contract=off)
        const float q = s1 * c2 + c1 * s2;                     // sin(b1 + b2)
        sum += c0 * p - s0 * q;                                // cos(b0 + b1 + b2)
      }
      dst[v] = src[v] + scale * sum;
    }
  } else {
    for (int i = tid; i < n; i += 256) dst[i0 + i] = src[i0 + i];
  }
}

// ---- two-tap gather along a per-sample axis --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void axis_gather2_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ srcs,
                                                           const float* __restrict__ wts, const int* __restrict__ axis,
                                                           const int* __restrict__ live, int n_max, int D, int H, int W) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int HW = H * W;
  const size_t V = (size_t)D * HW;
  const float* src = in + (size_t)b * V;
  float* dst = out + (size_t)b * V;
  const size_t i0 = (size_t)blockIdx.x * kGsChunk;
  const int n = (int)min((size_t)kGsChunk, V - i0);
  const int ax = __builtin_amdgcn_readfirstlane(axis[b]);
  if (!live[b] || ax < 0 || ax > 2) {
    for (int i = tid; i < n; i += 256) dst[i0 + i] = src[i0 + i];
    return;
  }
  const int N = ax == 0 ? D : ax == 1 ? H : W;
  const int stride = ax == 0 ? HW : ax == 1 ? W : 1;
  const int* st = srcs + (size_t)b * n_max * 2;
  const float* wt = wts + (size_t)b * n_max;
  for (int i = tid; i < n; i += 256) {                         // lanes along W: the two reads are coalesced for axes 0 and 1 and stay inside
    const size_t v = i0 + i;                                   // the lane's own line, in ascending order, for axis 2
    const int d = (int)(v / HW), r = (int)(v - (size_t)d * HW), h = r / W, w = r - h * W;
    const int j = ax == 0 ? d : ax == 1 ? h : w;
    const int j0 = min(max(st[2 * j], 0), N - 1), j1 = min(max(st[2 * j + 1], 0), N - 1);    // a bad table cannot read outside the volume
    const size_t o = v - (size_t)j * stride;
    const float x0 = src[o + (size_t)j0 * stride], x1 = src[o + (size_t)j1 * stride], wj = wt[j];
    dst[v] = wj == 0.f ? x0 : __builtin_fmaf(wj, x1 - x0, x0);
  }
}

}  // namespace gvk

extern "C" int gvk_axis_circular_conv(const float* in, float* out, const float* ctab, const int32_t* axis, const int32_t* live, int B, int D, int H,
                                      int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && ctab && axis && live, "gvk_axis_circular_conv: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && D > 0 && H > 0 && W > 0, "gvk_axis_circular_conv: bad shape");
  // axis is a device table this call does not read, so every extent a sample may convolve along has to be in range
  GVK_REQUIRE(D >= 2 && D <= kAcMaxN && H >= 2 && H <= kAcMaxN && W >= 2 && W <= kAcMaxN,
              "gvk_axis_circular_conv: volume (%d, %d, %d): 2..%d voxels on the convolved axis are built, and any axis may be drawn", D, H, W, kAcMaxN);
  GVK_REQUIRE(!ranges_overlap(in, out, (size_t)B * D * H * W * sizeof(float)), "gvk_axis_circular_conv: in and out must not overlap");
  const int n2 = (D * H + kAcLines - 1) / kAcLines, n1 = D * ((W + kAcCols - 1) / kAcCols), n0 = (H * W + kAcCols - 1) / kAcCols;
  const unsigned gx = (unsigned)max(n2, max(n1, n0));
  GVK_LAUNCH(axis_circular_conv_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, out, ctab, (const int*)axis, (const int*)live, D, H, W);
  return check_launch("axis_circular_conv");
}

extern "C" int gvk_gamma_spike(const float* in, float* out, const int32_t* kind, const float* gamma, const float* amp, const int32_t* nspikes,
                               const float* tab, const double* stats, int B, int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && kind && gamma && amp && nspikes && tab && stats, "gvk_gamma_spike: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < ((int64_t)1 << 31), "gvk_gamma_spike: bad shape");
  const size_t V = (size_t)D * H * W;
  GVK_REQUIRE(!ranges_overlap(in, out, (size_t)B * V * sizeof(float)), "gvk_gamma_spike: in and out must not overlap");
  const unsigned gx = (unsigned)((V + kGsChunk - 1) / kGsChunk);
  GVK_LAUNCH(gamma_spike_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, out, (const int*)kind, gamma, amp, (const int*)nspikes, tab, stats,
             D, H, W);
  return check_launch("gamma_spike");
}

extern "C" int gvk_axis_gather2(const float* in, float* out, const int32_t* src, const float* w, const int32_t* axis, const int32_t* live, int n_max,
                                int B, int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && src && w && axis && live, "gvk_axis_gather2: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < ((int64_t)1 << 31), "gvk_axis_gather2: bad shape");
  GVK_REQUIRE(n_max >= D && n_max >= H && n_max >= W, "gvk_axis_gather2: table rows of %d entries, the volume is (%d, %d, %d) and any axis may be drawn",
              n_max, D, H, W);
  const size_t V = (size_t)D * H * W;
  GVK_REQUIRE(!ranges_overlap(in, out, (size_t)B * V * sizeof(float)), "gvk_axis_gather2: in and out must not overlap (the kernel reads neighbouring voxels)");
  const unsigned gx = (unsigned)((V + kGsChunk - 1) / kGsChunk);
  GVK_LAUNCH(axis_gather2_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, out, (const int*)src, w, (const int*)axis, (const int*)live, n_max,
             D, H, W);
  return check_launch("axis_gather2");
}
