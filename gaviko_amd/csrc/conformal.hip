// Split-conformal prediction sets (gaviko_amd.metrics.conformal_scores / conformal_calibrate / conformal_evaluate).
//
// gvk_conformal_scores: the nonconformity score of every (row, class) from the probabilities -- lac (Sadinle et al., 2019), aps (Romano et
// al., 2020) and raps (Angelopoulos et al., 2021) -- written class-major, scores[k][n], because gvk_conformal_splits reads a class column
// with consecutive rows in consecutive lanes.  One wave per row, one class per lane, no atomics.  Every operation is ONE fp32 rounding (the
// library is built with -ffp-contract=off, and this file says so again): tests/conformal_ref.py restates it in numpy float32 bit for bit.
//
// gvk_conformal_splits: replicate b splits the N rows of an evaluation set at random into n_cal calibration rows and N - n_cal test rows,
// takes the conformal threshold of every segment (the whole set, or one per class: Mondrian) from the calibration rows, and counts the test
// rows' prediction sets.  With the rows sorted once per call by their TRUE-class score inside their segment (order, seg_off), the m-th
// smallest calibration score of a segment is one inclusive scan of the membership flags over `order`: the calibration row whose running
// count, less the count before its segment, is m.  Everything it leaves is an exact integer.
#include <math.h>

#include "replicate.hpp"
#include "../../include/gaviko_hip.h"

#pragma clang fp contract(off)

namespace gvk {

constexpr int kConfMaxN = GVK_BOOTSTRAP_MAX_ROWS;                // the row index takes the low 13 bits of a split key
constexpr int kConfMaxK = GVK_CONFORMAL_MAX_CLASSES;             // one class per lane of a wave
constexpr int kConfMaxQ = GVK_CONFORMAL_MAX_LEVELS;
constexpr unsigned int kConfRowMask = (unsigned int)kConfMaxN - 1u;
static_assert((kConfMaxN & (kConfMaxN - 1)) == 0, "the split key keeps the row index in its low bits");

// One wave per row (4 rows per 256-thread workgroup); lane k holds class k.
//   rank r_k = #{j : p_j > p_k or (p_j == p_k and j < k)}  (0-based; a permutation of 0..K-1 when no p is NaN)
//   lac:  s_k = 1 - p_k
//   aps:  c_0 = 0, c_{r+1} = c_r + p_pi(r) added in rank order;  s_pi(r) = c_{r+1}, or randomised  c_r + (u_n * p_pi(r))
//   raps: aps + (lam * float(max(0, r + 1 - k_reg)))
__global__ __launch_bounds__(256) void conformal_scores_kernel(const float* __restrict__ proba, float* __restrict__ scores, int N, int K, int kind,
                                                               int randomized, unsigned long long seed, int k_reg, float lam) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                                       // a whole wave leaves: the shuffles below see full waves only
  const bool live = lane < K;
  const float p = live ? proba[(size_t)n * K + lane] : 0.f;
  float s;
  if (kind == GVK_CONFORMAL_LAC) {
    s = 1.0f - p;
  } else {
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float pj = __shfl(p, j, 64);
      rank += (pj > p || (pj == p && j < lane)) ? 1 : 0;
    }
    if (!live) rank = 64 + lane;                                            // never a rank the loop below asks for
    float c = 0.f, before = 0.f, after = 0.f;
    for (int r = 0; r < K; ++r) {
      const unsigned long long who = __ballot(rank == r);
      const int src = who ? __ffsll((long long)who) - 1 : 0;                // no lane has the rank: NaN probabilities (the caller's contract)
      const float c1 = c + __shfl(p, src, 64);
      if (rank == r) { before = c; after = c1; }
      c = c1;
    }
    if (randomized) {
      const float u = (float)(hash_u32(seed, (unsigned long long)n) >> 8) * 0x1p-24f;
      const float up = u * p;
      s = before + up;
    } else {
      s = after;
    }
    if (kind == GVK_CONFORMAL_RAPS) {
      const int over = rank + 1 - k_reg;
      const float pen = lam * (float)(over > 0 ? over : 0);
      s = s + pen;
    }
  }
  if (live) scores[(size_t)lane * N + n] = s;
}

// the small tables of a replicate behind keys | P in the dynamic LDS, in 32-bit words (every offset a multiple of 4 words)
constexpr int kConfQG = kConfMaxQ * kConfMaxK;                   // [Q][G] tables
constexpr int kConfQS = (kConfMaxQ * (kConfMaxK + 1) + 3) / 4 * 4;   // [Q][K + 1] histograms
constexpr int kOffBins = 0;                                      // 256 radix bins
constexpr int kOffWave = kOffBins + 256;                         // 4 wave totals
constexpr int kOffSel = kOffWave + 4;                            // the bin a radix pass chose, and the rank left inside it
constexpr int kOffM = kOffSel + 4;                               // m [Q][G]
constexpr int kOffQhat = kOffM + kConfQG;                        // qhat [Q][G] (float)
constexpr int kOffQpos = kOffQhat + kConfQG;                     // qpos [Q][G]
constexpr int kOffBase = kOffQpos + kConfQG;                     // calibration rows before the segment [G]
constexpr int kOffNg = kOffBase + kConfMaxK;                     // calibration rows of the segment [G]
constexpr int kOffSize = kOffNg + kConfMaxK;                     // size_hist [Q][K + 1]
constexpr int kOffCovSize = kOffSize + kConfQS;                  // covered_by_size [Q][K + 1]
constexpr int kOffClsTest = kOffCovSize + kConfQS;               // class_test [K]
constexpr int kOffClsCov = kOffClsTest + kConfMaxK;              // class_covered [Q][K]
constexpr int kConfSmallWords = kOffClsCov + kConfQG;
static_assert(kConfSmallWords % 4 == 0, "the LDS carve keeps 16-byte alignment");

// One 256-thread workgroup per replicate.  LDS (dynamic): keys[Npad] | P[Npad] | the small tables above, Npad = N rounded up to the scan tile.
//   keys[i] = (hash_u32(seed, b N + i) & ~0x1FFF) | i: distinct, so "the n_cal rows with the smallest keys" is  keys[i] <= T  with T the
//             n_cal-th smallest key, found by a 4-pass radix select (8 bits per pass, 256 bins = one per thread, LDS atomics)
//   P[s]    = 1 if the row at sorted position s is a calibration row, then its inclusive scan (block_scan_tiles_u32 of replicate.hpp)
// Every index read from a table is clamped before it addresses LDS or global memory: the tables are the caller's contract
// (ops.conformal_tables builds them), a broken one gives wrong counts, never an access outside the arrays.  The histograms are LDS integer
// atomics; nothing is accumulated in global memory.
__global__ __launch_bounds__(256) void conformal_splits_kernel(const float* __restrict__ scores, const long long* __restrict__ labels,
                                                               const int* __restrict__ order, const int* __restrict__ seg_off,
                                                               const double* __restrict__ alphas, int* __restrict__ qpos, int* __restrict__ n_seg,
                                                               int* __restrict__ size_hist, int* __restrict__ covered_by_size,
                                                               int* __restrict__ class_test, int* __restrict__ class_covered, int N, int K, int Q,
                                                               int G, int Npad, int n_cal, unsigned long long seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned int conf_lds[];
  unsigned int* keys = conf_lds;
  unsigned int* P = conf_lds + Npad;
  unsigned int* small = conf_lds + 2 * Npad;
  unsigned int* s_bins = small + kOffBins;
  unsigned int* s_wave = small + kOffWave;
  unsigned int* s_sel = small + kOffSel;
  int* s_m = (int*)(small + kOffM);
  float* s_qhat = (float*)(small + kOffQhat);
  int* s_qpos = (int*)(small + kOffQpos);
  int* s_base = (int*)(small + kOffBase);
  int* s_ng = (int*)(small + kOffNg);
  unsigned int* s_size = small + kOffSize;
  unsigned int* s_covsize = small + kOffCovSize;
  unsigned int* s_clstest = small + kOffClsTest;
  unsigned int* s_clscov = small + kOffClsCov;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long b = blockIdx.x;
  const int K1 = K + 1;

  for (int i = t; i < N; i += 256)
    keys[i] = (hash_u32(seed, b * (unsigned long long)N + (unsigned long long)i) & ~kConfRowMask) | (unsigned int)i;
  for (int i = kOffM + t; i < kConfSmallWords; i += 256) small[i] = 0u;     // m, base, n_g and the histograms start at 0 ...
  __syncthreads();
  for (int i = t; i < Q * G; i += 256) { s_qhat[i] = INFINITY; s_qpos[i] = -1; }   // ... a threshold at +inf until a calibration row sets it

  // T = the n_cal-th smallest key: per pass, the bins of the next 8 bits among the keys that share the prefix found so far
  unsigned int prefix = 0u, mask = 0u, left = (unsigned int)n_cal;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_bins[t] = 0u;
    __syncthreads();
    for (int i = t; i < N; i += 256) {
      const unsigned int key = keys[i];
      if ((key & mask) == prefix) atomicAdd(&s_bins[(key >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    const unsigned int c = s_bins[t], inc = wave_scan_u32(c);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    const unsigned int incl = inc + (wave > 0 ? s_wave[0] : 0u) + (wave > 1 ? s_wave[1] : 0u) + (wave > 2 ? s_wave[2] : 0u);
    if (incl - c < left && left <= incl) { s_sel[0] = (unsigned int)t; s_sel[1] = left - (incl - c); }   // exactly one bin: 1 <= left <= the keys counted
    __syncthreads();
    prefix |= s_sel[0] << shift;
    mask |= 0xFFu << shift;
    left = s_sel[1];
  }
  const unsigned int T = prefix;                                            // keys[i] <= T: a calibration row (n_cal == N: every row)

  for (int s = t; s < Npad; s += 256) P[s] = (s < N && keys[clamp_row(order[s], N)] <= T) ? 1u : 0u;
  __syncthreads();
  block_scan_tiles_u32(P, Npad, s_wave);

  // per segment: the calibration rows before it and inside it; per level the order statistic asked for (0: none, the threshold stays +inf)
  for (int g = t; g < G; g += 256) {
    int o0 = seg_off[g], o1 = seg_off[g + 1];
    o0 = o0 < 0 ? 0 : (o0 > N ? N : o0);
    o1 = o1 < o0 ? o0 : (o1 > N ? N : o1);
    const int before = o0 > 0 ? (int)P[o0 - 1] : 0, upto = o1 > 0 ? (int)P[o1 - 1] : 0;
    s_base[g] = before;
    s_ng[g] = upto - before;
  }
  __syncthreads();
  for (int i = t; i < Q * G; i += 256) {
    const int q = i / G, g = i - q * G, ng = s_ng[g];
    int m = (int)ceil((double)(ng + 1) * (1.0 - alphas[q]));
    m = m < 1 ? 1 : m;                                                      // alpha outside (0, 1) is the caller's contract
    s_m[i] = m > ng ? 0 : m;
  }
  __syncthreads();
  for (int s = t; s < N; s += 256) {
    const int row = clamp_row(order[s], N);
    if (keys[row] > T) continue;
    const int yc = clamp_label(labels[row], K);                             // labels outside [0, K) are the caller's contract
    const int g = G == 1 ? 0 : yc;
    const int r = (int)P[s] - s_base[g];                                    // this row is the r-th calibration row of its segment, 1-based
    for (int q = 0; q < Q; ++q)
      if (s_m[q * G + g] == r) { s_qpos[q * G + g] = s; s_qhat[q * G + g] = scores[(size_t)yc * N + row]; }
  }
  __syncthreads();

  // the test rows: set sizes and coverage at every level
  for (int i = t; i < N; i += 256) {
    if (keys[i] <= T) continue;
    const int yc = clamp_label(labels[i], K);
    int size[kConfMaxQ];
#pragma unroll
    for (int q = 0; q < kConfMaxQ; ++q) size[q] = 0;
    float sy = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = scores[(size_t)k * N + i];
      const int g = G == 1 ? 0 : k;
      if (k == yc) sy = v;
#pragma unroll
      for (int q = 0; q < kConfMaxQ; ++q)
        if (q < Q) size[q] += v <= s_qhat[q * G + g] ? 1 : 0;
    }
    atomicAdd(&s_clstest[yc], 1u);
    const int gy = G == 1 ? 0 : yc;
#pragma unroll
    for (int q = 0; q < kConfMaxQ; ++q) {
      if (q < Q) {
        atomicAdd(&s_size[q * K1 + size[q]], 1u);
        if (sy <= s_qhat[q * G + gy]) {
          atomicAdd(&s_covsize[q * K1 + size[q]], 1u);
          atomicAdd(&s_clscov[q * K + yc], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int i = t; i < Q * G; i += 256) qpos[b * Q * G + i] = s_qpos[i];
  for (int i = t; i < G; i += 256) n_seg[b * G + i] = s_ng[i];
  for (int i = t; i < Q * K1; i += 256) {
    size_hist[b * Q * K1 + i] = (int)s_size[i];
    covered_by_size[b * Q * K1 + i] = (int)s_covsize[i];
  }
  for (int i = t; i < K; i += 256) class_test[b * K + i] = (int)s_clstest[i];
  for (int i = t; i < Q * K; i += 256) class_covered[b * Q * K + i] = (int)s_clscov[i];
}

}  // namespace gvk

extern "C" int gvk_conformal_scores(const float* proba, float* scores, int N, int K, int kind, int randomized, uint64_t seed, int k_reg, float lam,
                                    void* stream) {
  using namespace gvk;
  GVK_REQUIRE(proba && scores, "gvk_conformal_scores: bad arguments");
  GVK_REQUIRE(N >= 1, "gvk_conformal_scores: N = %d rows (at least 1)", N);
  GVK_REQUIRE(K >= 2 && K <= kConfMaxK, "gvk_conformal_scores: K = %d classes outside [2, %d] (one class per lane)", K, kConfMaxK);
  GVK_REQUIRE(kind == GVK_CONFORMAL_LAC || kind == GVK_CONFORMAL_APS || kind == GVK_CONFORMAL_RAPS,
              "gvk_conformal_scores: kind = %d (0 lac, 1 aps, 2 raps)", kind);
  GVK_REQUIRE(randomized == 0 || randomized == 1, "gvk_conformal_scores: randomized = %d (0 or 1)", randomized);
  GVK_REQUIRE(!(randomized && kind == GVK_CONFORMAL_LAC), "gvk_conformal_scores: lac has no randomised form");
  GVK_REQUIRE(kind != GVK_CONFORMAL_RAPS || (k_reg >= 0 && lam >= 0.f), "gvk_conformal_scores: raps needs k_reg >= 0 and lam >= 0 (got %d, %g)", k_reg,
              (double)lam);
  GVK_LAUNCH(conformal_scores_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0u, (hipStream_t)stream, proba, scores, N, K, kind, randomized,
             (unsigned long long)seed, k_reg, lam);
  return check_launch("conformal_scores");
}

extern "C" int gvk_conformal_splits(const float* scores, const void* labels, const int32_t* order, const int32_t* seg_off, const double* alphas,
                                    int32_t* qpos, int32_t* n_seg, int32_t* size_hist, int32_t* covered_by_size, int32_t* class_test,
                                    int32_t* class_covered, int N, int K, int Q, int G, int n_cal, int R, uint64_t seed, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(scores && labels && order && seg_off && alphas && qpos && n_seg && size_hist && covered_by_size && class_test && class_covered,
              "gvk_conformal_splits: bad arguments");
  GVK_REQUIRE(N >= 1 && N <= kConfMaxN, "gvk_conformal_splits: N = %d rows outside [1, %d] (one workgroup keeps the keys and the scan in LDS)", N,
              kConfMaxN);
  GVK_REQUIRE(K >= 2 && K <= kConfMaxK, "gvk_conformal_splits: K = %d classes outside [2, %d]", K, kConfMaxK);
  GVK_REQUIRE(Q >= 1 && Q <= kConfMaxQ, "gvk_conformal_splits: Q = %d levels outside [1, %d]", Q, kConfMaxQ);
  GVK_REQUIRE(G == 1 || G == K, "gvk_conformal_splits: G = %d segments (1: marginal, K = %d: one per class)", G, K);
  GVK_REQUIRE(n_cal >= 1 && n_cal <= N, "gvk_conformal_splits: n_cal = %d calibration rows outside [1, %d]", n_cal, N);
  GVK_REQUIRE(R >= 1, "gvk_conformal_splits: R = %d replicates (at least 1)", R);
  const int Npad = scan_pad(N);
  const size_t lds = sizeof(unsigned int) * ((size_t)2 * Npad + (size_t)kConfSmallWords);
  static size_t granted = 64 * 1024;                                        // what a launch may ask for without the attribute
  if (int rc = ensure_lds(&conformal_splits_kernel, lds, granted, "conformal_splits")) return rc;
  GVK_LAUNCH(conformal_splits_kernel, dim3((unsigned)R), dim3(256), (unsigned)lds, (hipStream_t)stream, scores, (const long long*)labels,
             (const int*)order, (const int*)seg_off, alphas, (int*)qpos, (int*)n_seg, (int*)size_hist, (int*)covered_by_size, (int*)class_test,
             (int*)class_covered, N, K, Q, G, Npad, n_cal, (unsigned long long)seed);
  return check_launch("conformal_splits");
}
