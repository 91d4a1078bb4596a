// Predictive uncertainty (gaviko_amd.uncertainty: Monte-Carlo dropout, flip test-time augmentation) and calibration (gaviko_amd.metrics).
//   tta_volumes       the HBM pass of a member sweep: out[o] = x[src[o]] mirrored along the axes named by flip[o], written straight into the
//                     engine's input slot.  flip = 0 is a plain replica (the members of MC-dropout).
//   predictive_stats  member logits [B][S][K] -> mean probabilities, prediction, the entropy decomposition, std, votes, variation ratio.
//   calibration_bins  probabilities [N][K] + labels -> reliability-diagram bins (count, correct, confidence sum), Brier and NLL sums.
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// out[o][z][y][x] = x[src[o]][fz][fy][fx] with fz = flip & 1 ? D - 1 - z : z, fy = flip & 2 ? H - 1 - y : y, fx = flip & 4 ? W - 1 - x : x.
// A move of 32-bit words, no arithmetic: the output carries the bits of its source.
// VEC = 4 (W % 4 == 0): one thread per 4 consecutive voxels along W, 16-byte loads and stores; the W mirror reads the mirrored float4 (it
// starts at W - 4 - x, again a multiple of 4) and reverses its four lanes.  VEC = 1: one thread per voxel, any geometry.
// Algorithmic bytes per launch: Bout * V * 4 written and as many read (every output voxel has one source voxel; the members that share a
// source re-read it from cache).  32-bit index arithmetic: the entry point checks that Bout * V fits.
template <int VEC>
__global__ __launch_bounds__(256) void tta_volumes_kernel(const uint32_t* __restrict__ x, const int* __restrict__ src, const int* __restrict__ flip,
                                                          uint32_t* __restrict__ out, int Bout, int S, int D, int H, int W) {
  const unsigned uH = H, uD = D, uW = W;
  const unsigned wq = uW / VEC;
  const int64_t V = (int64_t)D * H * W;
  const unsigned total = (unsigned)Bout * uD * uH * wq;
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const unsigned row = idx / wq, xq = idx - row * wq;         // row = (o * D + z) * H + y
    const unsigned oz = row / uH, y = row - oz * uH;
    const unsigned o = oz / uD, z = oz - o * uD;
    const unsigned xx = xq * VEC;
    int s = src[o];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);                       // the values are the caller's contract; clamped so that nothing outside x is read
    const int f = flip[o];
    const unsigned fz = (f & 1) ? uD - 1 - z : z, fy = (f & 2) ? uH - 1 - y : y;
    const uint32_t* in = x + (int64_t)s * V + (int64_t)(fz * uH + fy) * W;
    uint32_t* dst = out + (int64_t)o * V + (int64_t)(z * uH + y) * W + xx;
    if (VEC == 4) {
      u32x4 r;
      if (f & 4) {
        const u32x4 m = *(const u32x4*)(in + (uW - 4 - xx));
        r = u32x4{m.w, m.z, m.y, m.x};
      } else {
        r = *(const u32x4*)(in + xx);
      }
      *(u32x4*)dst = r;
    } else {
      *dst = in[(f & 4) ? uW - 1 - xx : xx];
    }
  }
}

constexpr int kStatsKPL = 4;                                    // classes per lane of predictive_stats_kernel
constexpr int kStatsMaxK = 64 * kStatsKPL;

// softmax of one member row over the wave: lane l holds the classes l, l + 64, ... (p[j] = class l + 64 j; classes >= K hold 0).  Returns
// the lowest index of the largest logit.  Called twice per member with the same inputs: the same bits both times.
__device__ __forceinline__ int member_softmax(const float* __restrict__ z, int K, int lane, float (&p)[kStatsKPL]) {
  float v[kStatsKPL];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) {
    const int k = lane + 64 * j;
    v[j] = k < K ? z[k] : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
  mx = wave_max(mx);
  int am = INT_MAX;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) {
    const int k = lane + 64 * j;
    if (k < K && v[j] == mx) am = min(am, k);
    p[j] = k < K ? expf(v[j] - mx) : 0.f;
    sum += p[j];
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) p[j] = p[j] / sum;
  return wave_min(am);
}

// H[p] = -sum_k p_k log p_k with 0 log 0 = 0; the xor butterfly leaves the same bits in every lane
__device__ __forceinline__ float wave_entropy(const float (&p)[kStatsKPL]) {
  float h = 0.f;
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) h += p[j] > 0.f ? -p[j] * logf(p[j]) : 0.f;
  return wave_sum(h);
}

// One wave per sample b (4 samples per workgroup, no LDS, no atomics, no barrier): the members are walked in s order, twice -- once for the
// mean, the member entropies and the votes, once more for the squared deviations from the mean (so that S = 1 gives std == 0 and
// mutual_info == 0 exactly: mean = p / 1, and both entropies are the same function of the same bits).  Every reduction is a fixed butterfly
// over the wave or a loop in s order: two runs are bit-identical.
__global__ __launch_bounds__(256) void predictive_stats_kernel(const float* __restrict__ logits, float* __restrict__ probs, int* __restrict__ pred,
                                                               float* __restrict__ entropy, float* __restrict__ expected_entropy,
                                                               float* __restrict__ mutual_info, float* __restrict__ variation_ratio,
                                                               float* __restrict__ stdev, int* __restrict__ votes, int B, int S, int K) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                           // uniform over the wave
  const float* zb = logits + (int64_t)b * S * K;
  float mean[kStatsKPL], p[kStatsKPL];
  int vote[kStatsKPL];
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) { mean[j] = 0.f; vote[j] = 0; }
  float hsum = 0.f;
  for (int s = 0; s < S; ++s) {
    const int am = member_softmax(zb + (int64_t)s * K, K, lane, p);
    hsum += wave_entropy(p);
#pragma unroll
    for (int j = 0; j < kStatsKPL; ++j) {
      mean[j] += p[j];
      vote[j] += (am == lane + 64 * j) ? 1 : 0;
    }
  }
  const float fS = (float)S;
  float top = -INFINITY;
  int vmax = 0;
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) {
    mean[j] = mean[j] / fS;
    if (lane + 64 * j < K) top = fmaxf(top, mean[j]);
    vmax = max(vmax, vote[j]);
  }
  top = wave_max(top);
  vmax = wave_max(vmax);
  int am = INT_MAX;
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j)
    if (lane + 64 * j < K && mean[j] == top) am = min(am, lane + 64 * j);
  am = wave_min(am);
  const float h = wave_entropy(mean), he = hsum / fS;
  float var[kStatsKPL];
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) var[j] = 0.f;
  for (int s = 0; s < S; ++s) {
    member_softmax(zb + (int64_t)s * K, K, lane, p);
#pragma unroll
    for (int j = 0; j < kStatsKPL; ++j) {
      const float d = p[j] - mean[j];
      var[j] += d * d;
    }
  }
#pragma unroll
  for (int j = 0; j < kStatsKPL; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      probs[(int64_t)b * K + k] = mean[j];
      stdev[(int64_t)b * K + k] = sqrtf(var[j] / fS);
      votes[(int64_t)b * K + k] = vote[j];
    }
  }
  if (lane == 0) {
    pred[b] = am < K ? am : 0;                                  // (NaN logits: no class equals the maximum)
    entropy[b] = h;
    expected_entropy[b] = he;
    mutual_info[b] = fmaxf(h - he, 0.f);
    variation_ratio[b] = 1.f - (float)vmax / fS;
  }
}

// One workgroup walks the rows in tiles of 256: thread t of a tile scores row t (confidence = max_k p, prediction = its lowest index, the
// bin ceil(conf * nbins) - 1 of (i / nbins, (i + 1) / nbins] -- exact in double for nbins < 2^29 -- the Brier and NLL terms in double) into
// LDS; then thread i < nbins adds the tile's rows of bin i in row order, thread nbins the Brier terms, thread nbins + 1 the NLL terms.  Every
// sum is therefore taken in row order whatever N: no atomics, two runs bit-identical.  N is an evaluation set (hundreds to thousands of rows).
__global__ __launch_bounds__(256) void calibration_bins_kernel(const float* __restrict__ proba, const long long* __restrict__ target,
                                                               long long* __restrict__ count, long long* __restrict__ correct,
                                                               double* __restrict__ conf_sum, double* __restrict__ brier, double* __restrict__ nll,
                                                               int N, int K, int nbins) {
  __shared__ float s_conf[256];
  __shared__ int s_bin[256];                                    // bit 30: the prediction is correct
  __shared__ double s_brier[256], s_nll[256];
  const int t = threadIdx.x;
  long long cnt = 0, cor = 0;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += 256) {
    const int n = n0 + t;
    if (n < N) {
      const float* p = proba + (int64_t)n * K;
      const long long y = target[n];
      float c = p[0];
      int am = 0;
      double br = 0.0;
      for (int k = 0; k < K; ++k) {
        if (p[k] > c) { c = p[k]; am = k; }
        const double d = (double)p[k] - (y == k ? 1.0 : 0.0);
        br += d * d;
      }
      int bin = (int)ceil((double)c * (double)nbins) - 1;
      bin = bin < 0 ? 0 : (bin >= nbins ? nbins - 1 : bin);     // conf == 0 (or NaN) goes to the first bin
      s_conf[t] = c;
      s_bin[t] = bin | ((long long)am == y ? (1 << 30) : 0);
      s_brier[t] = br;
      s_nll[t] = (y >= 0 && y < K) ? -log((double)fmaxf(p[y], FLT_MIN)) : 0.0;   // a label outside [0, K) has no probability: the caller rejects it
    }
    __syncthreads();
    const int lim = min(256, N - n0);
    if (t < nbins) {
      for (int r = 0; r < lim; ++r) {
        const int bb = s_bin[r];
        if ((bb & ((1 << 30) - 1)) == t) {
          cnt += 1;
          cor += bb >> 30;
          acc += (double)s_conf[r];
        }
      }
    } else if (t == nbins) {
      for (int r = 0; r < lim; ++r) acc += s_brier[r];
    } else if (t == nbins + 1) {
      for (int r = 0; r < lim; ++r) acc += s_nll[r];
    }
    __syncthreads();
  }
  if (t < nbins) {
    count[t] = cnt;
    correct[t] = cor;
    conf_sum[t] = acc;
  } else if (t == nbins) {
    brier[0] = acc;
  } else if (t == nbins + 1) {
    nll[0] = acc;
  }
}

}  // namespace gvk

extern "C" int gvk_tta_volumes(const float* x, const int32_t* src, const int32_t* flip, float* out, int Bout, int S, int D, int H, int W, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && src && flip && out && Bout > 0 && S > 0 && D > 0 && H > 0 && W > 0, "gvk_tta_volumes: bad arguments");
  const int64_t V = (int64_t)D * H * W;
  GVK_REQUIRE((int64_t)Bout * V < (1LL << 31), "gvk_tta_volumes: %d x %lld voxels per launch exceed the 32-bit index range", Bout, (long long)V);
  GVK_REQUIRE(out + (int64_t)Bout * V <= x || x + (int64_t)S * V <= out, "gvk_tta_volumes: out must not overlap x");
  const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  if (vec)
    GVK_LAUNCH(tta_volumes_kernel<4>, dim3(grid_blocks((int64_t)Bout * V / 4, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)x, (const int*)src,
               (const int*)flip, (uint32_t*)out, Bout, S, D, H, W);
  else
    GVK_LAUNCH(tta_volumes_kernel<1>, dim3(grid_blocks((int64_t)Bout * V, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)x, (const int*)src,
               (const int*)flip, (uint32_t*)out, Bout, S, D, H, W);
  return check_launch("tta_volumes");
}

extern "C" int gvk_predictive_stats(const float* member_logits, float* probs, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info,
                                    float* variation_ratio, float* std, int32_t* votes, int B, int S, int K, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(member_logits && probs && pred && entropy && expected_entropy && mutual_info && variation_ratio && std && votes && B > 0,
              "gvk_predictive_stats: bad arguments");
  GVK_REQUIRE(S >= 1, "gvk_predictive_stats: S = %d members (at least 1)", S);
  GVK_REQUIRE(K >= 2 && K <= kStatsMaxK, "gvk_predictive_stats: K = %d classes outside [2, %d] (one wave keeps %d classes per lane in registers)", K,
              kStatsMaxK, kStatsKPL);
  GVK_LAUNCH(predictive_stats_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, member_logits, probs, (int*)pred, entropy,
             expected_entropy, mutual_info, variation_ratio, std, (int*)votes, B, S, K);
  return check_launch("predictive_stats");
}

extern "C" int gvk_calibration_bins(const float* proba, const void* target, int64_t* count, int64_t* correct, double* conf_sum, double* brier, double* nll,
                                    int N, int K, int nbins, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(proba && target && count && correct && conf_sum && brier && nll && N > 0 && K > 0, "gvk_calibration_bins: bad arguments");
  GVK_REQUIRE(nbins >= 1 && nbins <= 254, "gvk_calibration_bins: nbins = %d outside [1, 254] (one thread of the workgroup per bin)", nbins);
  GVK_LAUNCH(calibration_bins_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, proba, (const long long*)target, (long long*)count,
             (long long*)correct, conf_sum, brier, nll, N, K, nbins);
  return check_launch("calibration_bins");
}
