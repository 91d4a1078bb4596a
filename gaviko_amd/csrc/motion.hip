// tio.RandomMotion on the device: the fourth member of the intensity group train.py:43-48 declares, k-space motion ghosting of a batch of
// fp32 volumes [B][D][H][W] already in HBM, in ONE fused pass and without an FFT.
//
// torchio resamples the volume under K rigid movements, takes the shifted 3-D spectrum of the original and of every moved copy and
// composites them in K+1 slabs along the LAST array axis (slab edges int(W t_k), source order by its sort_spectra), then transforms back
// and keeps the real part.  The slab masks do not depend on the other two frequency axes, so the transforms over D and H cancel against
// their inverses; along W a slab mask is a real circular convolution (the slabs are symmetric up to the real part that is kept).  What is
// left is   y[d][h][w] = sum_{s=0..K} sum_{w'} c_s[(w - w') mod W] img_s[d][h][w'],   c_s[m] = (1/W) sum_{j in slabs of s} cos(2 pi (j - W/2) m / W) (W/2 the integer quotient, also for odd W),
// with the K+1 rows c_s built on the host in float64 (data.motion_tables); they sum to the unit impulse.  The same move as evp.hip's
// high-pass filter.  Pinned against the literal np.fft algorithm (tests/motion_ref.py); parity with torchio itself is unpinned.
//
// The kernel is a [lines x (K+1) W] by [(K+1) W x W] product whose left operand is made on the fly: a workgroup owns 32 consecutive (d, h)
// lines of one sample; per image s it gathers those lines into LDS -- the plain line for s = 0, the trilinear resample through movement s
// for the others (resample.hpp: the arithmetic of gvk_spatial_transform) -- beside a doubled copy of c_s, from which every lane reads its
// element of the circulant at the offset w - w'.  The product runs on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: fp32 operands,
// one rounding per product, fp32 accumulation in k order = an fmaf chain; bf16 operands would not do, the rows cancel to an impulse on raw
// intensities of ~1e3), image after image into the same accumulators, so the moved images never exist in HBM and every output line is
// written once.  2 (K+1) W flops per voxel: 11.8 GFLOP at B = 4, (120,160,160), K = 2 against ~100 MB of traffic -- bound by the matrix pipe.
#include "circulant.hpp"
#include "resample.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kMoLines = 32;                                   // lines per workgroup: two 16-row tiles, one per wave parity
constexpr int kMoMaxW = GVK_MOTION_MAX_W;
constexpr int kMoMaxStride = kMoMaxW + 2;
static_assert(kMoMaxW == 256, "gvk_motion_artifact lists 1..8 column tiles per wave");
static_assert(circulant_stride(kMoMaxW) == kMoMaxStride, "s_x holds 32 lines at the widest stride");

// Global accesses of whole lines (plain line, dead-sample copy, output) are one dword per lane: the live path is bound by the matrix pipe,
// not by these streams.  The product is circulant.hpp's; NT = ceil(column tiles / 2) is a template argument so that its loop has no branch.
template <int NT>
__global__ __launch_bounds__(256) void motion_artifact_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ mats,
                                                              const float* __restrict__ ctab, const int* __restrict__ live,
                                                              const float* __restrict__ part, int K, int D, int H, int W) {
  __shared__ float s_x[kMoLines * kMoMaxStride];               // the lines of one image, then the output tile
  __shared__ float s_c[2 * kMoMaxW + 16];                      // s_c[i] = c_s[(i - Wk) mod W]: the circulant at offset w - w' + Wk
  const int b = blockIdx.y;
  const int DH = D * H;
  const int line0 = blockIdx.x * kMoLines;
  const int nlines = min(kMoLines, DH - line0);
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const float* src = in + (size_t)b * DH * W;
  float* dst = out + (size_t)b * DH * W;
  if (!live[b]) {                                              // block-uniform: this sample drew nothing, its bits pass through
    const size_t o = (size_t)line0 * W;
    for (int i = tid; i < nlines * W; i += 256) dst[o + i] = src[o + i];
    return;
  }
  float pad, hi_unused;
  reduce_partials(part, b, pad, hi_unused);
  const int Wk = (W + 15) & ~15, W4 = (W + 3) & ~3;            // columns of the output tiles; k extent of the product (columns W.. stay zero)
  const int S = circulant_stride(Wk);
  for (int i = tid; i < kMoLines * S; i += 256) s_x[i] = 0.f;  // lines past the volume and columns past W contribute nothing
  const int rt = wave & 1, ct0 = wave >> 1;
  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s <= K; ++s) {
    __syncthreads();                                           // the zero fill, or the previous image's product, is done with s_x and s_c
    const float* c = ctab + ((size_t)b * (K + 1) + s) * W;
    circulant_fill_row(s_c, c, W, Wk, tid);
    const float* m = mats + ((size_t)b * K + max(s - 1, 0)) * 12;
    for (int r = wave; r < nlines; r += 4) {                   // a wave per line, lanes along W: coalesced
      const int line = line0 + r;
      const int d = line / H, h = line - d * H;
      for (int w = lane; w < W; w += 64)
        s_x[r * S + w] = s == 0 ? src[(size_t)line * W + w] : trilinear_sample(src, m, (float)d, (float)h, (float)w, D, H, W, pad);
    }
    __syncthreads();
    circulant_product<NT>(acc, NT, s_x, S, s_c, Wk, W4, rt, ct0, lane);
  }
  circulant_store_lines<NT>(acc, NT, s_x, S, dst, line0, nlines, W, Wk, rt, ct0, wave, lane);
}

}  // namespace gvk

extern "C" int gvk_motion_artifact(const float* in, float* out, const float* mats, const float* ctab, const int32_t* live, const float* partials, int K,
                                   int B, int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(in && out && mats && ctab && live && partials, "gvk_motion_artifact: null pointer");
  GVK_REQUIRE(K >= 1 && K <= GVK_MOTION_MAX_TRANSFORMS, "gvk_motion_artifact: %d movements (1..%d are built)", K, GVK_MOTION_MAX_TRANSFORMS);
  GVK_REQUIRE(W >= 2 && W <= GVK_MOTION_MAX_W, "gvk_motion_artifact: last axis of %d voxels (2..%d are built)", W, GVK_MOTION_MAX_W);
  GVK_REQUIRE(B > 0 && D > 0 && H > 0 && B <= 65535 && (int64_t)D * H < (1ll << 30), "gvk_motion_artifact: bad shape");
  GVK_REQUIRE(!ranges_overlap(in, out, (size_t)B * D * H * W * sizeof(float)),
              "gvk_motion_artifact: in and out must not overlap (the kernel reads neighbouring lines)");
  const unsigned gx = (unsigned)(((int64_t)D * H + kMoLines - 1) / kMoLines);
  switch ((W + 31) / 32) {                                     // column tiles per wave
#define GVK_MOTION_CASE(NT)                                                                                                                       \
  case NT:                                                                                                                                        \
    GVK_LAUNCH(motion_artifact_kernel<NT>, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, in, out, mats, ctab, (const int*)live, partials, K, D, H, W); \
    break;
    GVK_MOTION_CASE(1) GVK_MOTION_CASE(2) GVK_MOTION_CASE(3) GVK_MOTION_CASE(4) GVK_MOTION_CASE(5) GVK_MOTION_CASE(6) GVK_MOTION_CASE(7)
    GVK_MOTION_CASE(8)
#undef GVK_MOTION_CASE
    default: return set_error(-2, "gvk_motion_artifact: last axis of %d voxels (2..%d are built)", W, GVK_MOTION_MAX_W);
  }
  return check_launch("motion_artifact");
}
