// Selective prediction and temperature scaling (gaviko_amd.metrics.risk_coverage / fit_temperature).
//
// gvk_risk_coverage: the risk-coverage curve of a confidence score (Geifman & El-Yaniv, 2017), for the full sample and for bootstrap
// replicates drawn by the rule of gvk_bootstrap_counts.  With the rows sorted once per call by DESCENDING score (order, and per sorted
// position the end gend of its group of equal scores), a replicate with integer multiplicities w on the rows is one inclusive scan:
//   position s carries  w << 16 | (w if its row is wrong else 0);  w sums to N <= 8192 = 2^13, so neither half ever reaches the other and one
//   32-bit scan gives both running sums (C, E) = (accepted rows, errors among them) at every position.
// A group of equal scores is accepted together: its (C_g, E_g) is the scan at its last position gend - 1, and its own weight c_g is the
// difference of C to the group before.  The first position of every group adds the group's term c_g E_g / C_g to aurc (c_g E_g < 2^26: one
// rounding, in the division) and answers the need[] entries that fall into (C_{g-1}, C_g].
//
// gvk_temperature_fit: one workgroup minimises the mean NLL of softmax(beta z) over beta = 1 / T by safeguarded Newton, float64 throughout,
// without a host read: every thread holds the same sums (the partials go through LDS and every thread adds them in the same order), so the
// whole iteration is uniform control flow.
#include "replicate.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kSelMaxN = GVK_BOOTSTRAP_MAX_ROWS;                 // multiplicities and their sums stay below 2^16: two of them share a word
constexpr int kSelMaxK = GVK_BOOTSTRAP_MAX_CLASSES;
constexpr int kSelMaxQ = GVK_RISK_COVERAGE_MAX_NEEDS;

// One 256-thread workgroup per replicate.  LDS (dynamic): w[Npad] | P[Npad], Npad = N rounded up to the scan tile.
//   w[row] = multiplicity of the row (the N draws add 1 each by 32-bit LDS atomics; all 1 when resample = 0)
//   P[s]   = the packed pair of the row at sorted position s, then its inclusive scan (block_scan_tiles_u32 of replicate.hpp)
// Every index read from a table is clamped before it addresses LDS or global memory: the tables are the caller's contract
// (ops.selective_tables builds them), a broken one gives wrong counts, never an access outside the arrays.  No atomics on global memory; the
// aurc partials are added in a fixed order (per thread by ascending position, the xor butterfly of a wave, the 4 waves in order).
__global__ __launch_bounds__(256) void risk_coverage_kernel(const long long* __restrict__ labels, const int* __restrict__ pred,
                                                            const int* __restrict__ order, const int* __restrict__ gend,
                                                            const int* __restrict__ class_rows, const int* __restrict__ class_off,
                                                            const int* __restrict__ need, double* __restrict__ aurc, int* __restrict__ at,
                                                            int* __restrict__ total, int* __restrict__ accepted, int* __restrict__ errors, int N,
                                                            int K, int Q, int Npad, unsigned long long seed, int stratified, int resample) {
  extern __shared__ __attribute__((aligned(16))) unsigned int sel_lds[];
  __shared__ unsigned int s_wave[4];
  __shared__ double s_red[4];
  __shared__ int s_need[kSelMaxQ];
  unsigned int* w = sel_lds;
  unsigned int* P = sel_lds + Npad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long b = blockIdx.x;

  for (int i = t; i < N; i += 256) w[i] = resample ? 0u : 1u;
  if (t < Q) {
    const int q = need[t];
    s_need[t] = q < 1 ? 1 : (q > N ? N : q);                               // within [1, N]: exactly one group answers it
  }
  __syncthreads();
  if (resample) {
    for (int n = t; n < N; n += 256) atomicAdd(&w[draw_row(seed, b, n, N, K, labels, class_rows, class_off, stratified)], 1u);
    __syncthreads();
  }
  for (int s = t; s < Npad; s += 256) {
    unsigned int v = 0u;
    if (s < N) {
      const int row = clamp_row(order[s], N);
      const unsigned int m = w[row];
      v = m << 16 | ((long long)pred[row] != labels[row] ? m : 0u);
    }
    P[s] = v;
  }
  __syncthreads();
  const unsigned int carry = block_scan_tiles_u32(P, Npad, s_wave);
  double acc = 0.0;
  for (int s = t; s < N; s += 256) {
    int ge = gend[s];
    ge = ge < s + 1 ? s + 1 : (ge > N ? N : ge);                            // a group ends at or after its own position
    const unsigned int g = P[ge - 1];
    const int Cg = (int)(g >> 16), Eg = (int)(g & 0xFFFFu);
    if (accepted) { accepted[s] = Cg; errors[s] = Eg; }
    int first = 1;
    if (s > 0) {
      const int gp = gend[s - 1];
      first = gp <= s;                                                      // the position before belongs to a group that ends here
    }
    if (first) {
      const int Cp = s > 0 ? (int)(P[s - 1] >> 16) : 0;
      const int cg = Cg - Cp;
      if (cg > 0) {                                                         // a group no draw reached is not a threshold
        acc += (double)((long long)cg * (long long)Eg) / (double)Cg;
        for (int q = 0; q < Q; ++q) {
          const int nq = s_need[q];
          if (Cp < nq && nq <= Cg) { at[(b * Q + q) * 2] = Cg; at[(b * Q + q) * 2 + 1] = Eg; }
        }
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s_red[wave] = acc;
  __syncthreads();
  if (t == 0) {
    aurc[b] = (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)N;
    total[b * 2] = (int)(carry >> 16);
    total[b * 2 + 1] = (int)(carry & 0xFFFFu);
  }
}

constexpr int kFitThreads = 1024;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitMaxIter = 64;

// the block's sum of three per-thread doubles, the same bits in every thread: the xor butterfly of a wave, then the 16 wave partials in order
__device__ __forceinline__ void fit_block_sum(double& a, double& b, double& c, double (*s_part)[3]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  a = wave_sum(a), b = wave_sum(b), c = wave_sum(c);
  __syncthreads();                                                          // the partials of the evaluation before have been read
  if (lane == 0) { s_part[wave][0] = a; s_part[wave][1] = b; s_part[wave][2] = c; }
  __syncthreads();
  a = b = c = 0.0;
  for (int i = 0; i < kFitWaves; ++i) { a += s_part[i][0]; b += s_part[i][1]; c += s_part[i][2]; }
}

// f'(beta), f''(beta) and the mean NLL at beta: thread t takes the rows t, t + 1024, ... in order.  Per row, with d_k = z_k - max z <= 0
// and e_k = exp(beta d_k):  S0 = sum e, S1 = sum e d, S2 = sum e d^2;  f' term = S1 / S0 - d_y,  f'' term = S2 / S0 - (S1 / S0)^2
// (the variance is the same for z and d),  NLL term = log S0 - beta d_y.
__device__ __forceinline__ void fit_eval(const float* __restrict__ logits, const long long* __restrict__ target, int N, int K, double beta,
                                         double (*s_part)[3], double& g, double& h, double& nll) {
  double sg = 0.0, sh = 0.0, sn = 0.0;
  for (int n = threadIdx.x; n < N; n += kFitThreads) {
    const float* z = logits + (size_t)n * K;
    float mf = z[0];
    for (int k = 1; k < K; ++k) mf = fmaxf(mf, z[k]);
    const double m = (double)mf;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const double d = (double)z[k] - m, e = exp(beta * d);
      S0 += e; S1 += e * d; S2 += e * d * d;
    }
    const long long y = target[n];
    const int yc = clamp_label(y, K);                                       // labels outside [0, K) are the caller's contract
    const double dy = (double)z[yc] - m, mean = S1 / S0, var = S2 / S0 - mean * mean;
    sg += mean - dy;
    sh += var > 0.0 ? var : 0.0;
    sn += log(S0) - beta * dy;
  }
  fit_block_sum(sg, sh, sn, s_part);
  g = sg / (double)N; h = sh / (double)N; nll = sn / (double)N;
}

__global__ __launch_bounds__(kFitThreads) void temperature_fit_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                                      double* __restrict__ state, int N, int K, double t_min, double t_max) {
  __shared__ double s_part[kFitWaves][3];
  double lo = 1.0 / t_max, hi = 1.0 / t_min;
  double g, h, nll, g1 = 0.0, h1 = 0.0, nll_before = 0.0, beta = 1.0, delta = 0.0, T;
  int it = 0, flags = 0, phase = 0;                                          // phases: f at beta = 1, at 1 / t_min, at 1 / t_max, Newton start, Newton
  for (;;) {                                                                // one call site: every thread takes the same path (g, h are uniform)
    fit_eval(logits, target, N, K, beta, s_part, g, h, nll);
    if (phase == 0) { g1 = g; h1 = h; nll_before = nll; beta = hi; phase = 1; continue; }
    if (phase == 1) {
      if (g <= 0.0) { T = t_min; flags = 3; break; }                        // still descending at the sharpest end of the bracket
      beta = lo; phase = 2; continue;
    }
    if (phase == 2) {
      if (g >= 0.0) { T = t_max; flags = 3; break; }                        // already ascending at the flattest end
      beta = 1.0 < lo ? lo : (1.0 > hi ? hi : 1.0);
      phase = 3;
      if (beta != 1.0) continue;
      g = g1; h = h1; nll = nll_before;                                     // beta = 1 lies in the bracket and is evaluated already
    }
    // converged: the step that led here, or the Newton step proposed from here, is within 2^-40 beta.  (The second test matters: a step of
    // 1e-10 beta that lands on the root leaves a proposal below one ulp, which would count as leaving the bracket and start a bisection.)
    const double step = h > 0.0 ? -g / h : hi - lo;
    if (g == 0.0 || (phase == 4 && fabs(delta) <= 0x1p-40 * beta) || fabs(step) <= 0x1p-40 * beta) { T = 1.0 / beta; flags = 1; break; }
    if (it >= kFitMaxIter) { T = 1.0 / beta; break; }
    if (g > 0.0) hi = beta; else lo = beta;                                 // f' ascends: its sign says on which side the minimum lies
    double nb = beta + step;
    if (!(nb > lo && nb < hi)) nb = 0.5 * (lo + hi);                        // a step out of the bracket (or f'' = 0, or NaN): bisect
    delta = nb - beta;
    beta = nb;
    ++it;
    phase = 4;
  }
  if (threadIdx.x == 0) {
    state[0] = T; state[1] = beta; state[2] = nll_before; state[3] = nll;
    state[4] = g; state[5] = h; state[6] = (double)it; state[7] = (double)flags;
  }
}

}  // namespace gvk

extern "C" int gvk_risk_coverage(const void* labels, const int32_t* pred, const int32_t* order, const int32_t* gend, const int32_t* class_rows,
                                 const int32_t* class_off, const int32_t* need, double* aurc, int32_t* at, int32_t* total, int32_t* accepted,
                                 int32_t* errors, int N, int K, int Q, int R, uint64_t seed, int stratified, int resample, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(labels && pred && order && gend && aurc && total, "gvk_risk_coverage: bad arguments");
  GVK_REQUIRE(N >= 1 && N <= kSelMaxN, "gvk_risk_coverage: N = %d rows outside [1, %d] (one workgroup keeps the multiplicities and the scan in LDS)", N,
              kSelMaxN);
  GVK_REQUIRE(Q >= 0 && Q <= kSelMaxQ, "gvk_risk_coverage: Q = %d accepted-row counts outside [0, %d]", Q, kSelMaxQ);
  GVK_REQUIRE(Q == 0 || (need && at), "gvk_risk_coverage: Q = %d needs the need and at arrays", Q);
  GVK_REQUIRE(R >= 1, "gvk_risk_coverage: R = %d replicates (at least 1)", R);
  GVK_REQUIRE(resample == 0 || resample == 1, "gvk_risk_coverage: resample = %d (0 or 1)", resample);
  GVK_REQUIRE(stratified == 0 || stratified == 1, "gvk_risk_coverage: stratified = %d (0 or 1)", stratified);
  GVK_REQUIRE(resample || R == 1, "gvk_risk_coverage: resample = 0 is the full sample, R = %d must be 1", R);
  GVK_REQUIRE(!(resample && stratified) || (class_rows && class_off && K >= 1 && K <= kSelMaxK),
              "gvk_risk_coverage: the stratified rule needs class_rows, class_off and 1 <= K <= %d (K = %d)", kSelMaxK, K);
  GVK_REQUIRE((accepted == nullptr) == (errors == nullptr), "gvk_risk_coverage: accepted and errors come together");
  GVK_REQUIRE(!resample || !accepted, "gvk_risk_coverage: the curve (accepted, errors) is written with resample = 0 only");
  const int Npad = scan_pad(N);
  const size_t lds = sizeof(unsigned int) * (size_t)2 * Npad;
  static size_t granted = 64 * 1024 - 256;                                  // what a launch may ask for without the attribute (the static arrays take a little)
  if (int rc = ensure_lds(&risk_coverage_kernel, lds, granted, "risk_coverage")) return rc;
  GVK_LAUNCH(risk_coverage_kernel, dim3((unsigned)R), dim3(256), (unsigned)lds, (hipStream_t)stream, (const long long*)labels, (const int*)pred,
             (const int*)order, (const int*)gend, (const int*)class_rows, (const int*)class_off, (const int*)need, aurc, (int*)at, (int*)total,
             (int*)accepted, (int*)errors, N, K, Q, Npad, (unsigned long long)seed, stratified, resample);
  return check_launch("risk_coverage");
}

extern "C" int gvk_temperature_fit(const float* logits, const void* target, double* state, int N, int K, double t_min, double t_max, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(logits && target && state, "gvk_temperature_fit: bad arguments");
  GVK_REQUIRE(N >= 1, "gvk_temperature_fit: N = %d rows (at least 1)", N);
  GVK_REQUIRE(K >= 2 && K <= GVK_TEMPERATURE_MAX_CLASSES, "gvk_temperature_fit: K = %d classes outside [2, %d]", K, GVK_TEMPERATURE_MAX_CLASSES);
  GVK_REQUIRE(t_min > 0.0 && t_min < t_max && t_max <= 1.7e308, "gvk_temperature_fit: need 0 < t_min < t_max, finite (got %g, %g)", t_min, t_max);
  GVK_LAUNCH(temperature_fit_kernel, dim3(1), dim3(kFitThreads), 0u, (hipStream_t)stream, logits, (const long long*)target, state, N, K, t_min, t_max);
  return check_launch("temperature_fit");
}
