// ROC operating points of a binary reading (gaviko_amd.metrics.roc_analysis / roc_compare).
//
// gvk_roc_replicates: the ROC curve of a score against a binary label, for the full sample and for bootstrap replicates drawn by the rule
// of gvk_bootstrap_counts.  With the rows sorted once per call by DESCENDING score (order, and per sorted position the end gend of its group
// of equal scores), a replicate with integer multiplicities w on the rows is one inclusive scan:
//   position s carries  w << 16  for a positive row and  w  for a negative one;  w sums to N <= 8192 = 2^13, so neither half ever reaches the
//   other and one 32-bit scan gives both running sums (TP, FP) at every position.
// A group of equal scores is one point of the curve: its (TP_g, FP_g) is the scan at its last position gend - 1, its own (tp_g, fp_g) the
// difference to the scan at the position before its first.  The first position of every group adds the group's terms to auc2 and ap, takes
// part in the Youden maximum and answers the level lists by LOCAL tests: both searches are monotone in g, so exactly one group sees the
// predicate change between itself and its neighbour (the group before for at_sens, the group after for at_spec).  A group that no draw
// reached repeats the counts of the group before, so it never sees a change the group before did not see first.
#include "replicate.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kRocMaxN = GVK_BOOTSTRAP_MAX_ROWS;                 // multiplicities and their sums stay below 2^16: two of them share a word
constexpr int kRocMaxK = GVK_BOOTSTRAP_MAX_CLASSES;
constexpr int kRocMaxQ = GVK_ROC_MAX_LEVELS;
constexpr int kRocBp = 10000;                                    // levels are basis points: (Nn - FP) * 10000 and a * Nn stay below 2^27

__device__ __forceinline__ int roc_group_end(const int* __restrict__ gend, int s, int N) {
  const int ge = gend[s];
  return ge < s + 1 ? s + 1 : (ge > N ? N : ge);                            // a group ends at or after its own position
}

// One 256-thread workgroup per replicate.  LDS (dynamic): w[Npad] | P[Npad], Npad = N rounded up to the scan tile.
//   w[row] = multiplicity of the row (the N draws add 1 each by 32-bit LDS atomics; all 1 when resample = 0)
//   P[s]   = the packed pair of the row at sorted position s, then its inclusive scan (block_scan_tiles_u32 of replicate.hpp)
// Every index read from a table is clamped before it addresses LDS or global memory: the tables are the caller's contract (ops.roc_tables
// builds them), a broken one gives wrong counts, never an access outside the arrays.  No atomics on global memory.  auc2 is an integer sum;
// the ap partials are added in a fixed order (per thread by ascending position, the xor butterfly of a wave, the 4 waves in order); the
// Youden maximum is a maximum of distinct 64-bit keys: none of the three depends on scheduling.
__global__ __launch_bounds__(256) void roc_replicates_kernel(const long long* __restrict__ strata, const int* __restrict__ positive,
                                                             const int* __restrict__ order, const int* __restrict__ gend,
                                                             const int* __restrict__ class_rows, const int* __restrict__ class_off,
                                                             const int* __restrict__ spec_bp, const int* __restrict__ sens_bp,
                                                             const int* __restrict__ cut_rows, int* __restrict__ total,
                                                             long long* __restrict__ auc2, double* __restrict__ ap, int* __restrict__ at_spec,
                                                             int* __restrict__ at_sens, int* __restrict__ at_cut, int* __restrict__ youden,
                                                             int* __restrict__ tp_curve, int* __restrict__ fp_curve, int N, int K, int Qspec,
                                                             int Qsens, int Qcut, int Npad, unsigned long long seed, int stratified, int resample) {
  extern __shared__ __attribute__((aligned(16))) unsigned int roc_lds[];
  __shared__ unsigned int s_wave[4];
  __shared__ double s_red[4];
  __shared__ long long s_auc[4];
  __shared__ unsigned long long s_key[4];
  __shared__ int s_spec[kRocMaxQ], s_sens[kRocMaxQ];
  unsigned int* w = roc_lds;
  unsigned int* P = roc_lds + Npad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long b = blockIdx.x;

  for (int i = t; i < N; i += 256) w[i] = resample ? 0u : 1u;
  if (t < Qspec) {
    const int a = spec_bp[t];
    s_spec[t] = a < 0 ? 0 : (a > kRocBp ? kRocBp : a);
  }
  if (t < Qsens) {
    const int a = sens_bp[t];
    s_sens[t] = a < 0 ? 0 : (a > kRocBp ? kRocBp : a);
  }
  __syncthreads();
  if (resample) {
    for (int n = t; n < N; n += 256) atomicAdd(&w[draw_row(seed, b, n, N, K, strata, class_rows, class_off, stratified)], 1u);
    __syncthreads();
  }
  for (int s = t; s < Npad; s += 256) {
    unsigned int v = 0u;
    if (s < N) {
      const int row = clamp_row(order[s], N);
      const unsigned int m = w[row];
      v = positive[row] != 0 ? m << 16 : m;
    }
    P[s] = v;
  }
  __syncthreads();
  const unsigned int carry = block_scan_tiles_u32(P, Npad, s_wave);
  const int Pn = (int)(carry >> 16), Nn = (int)(carry & 0xFFFFu);
  double acc = 0.0;
  long long pairs = 0;
  unsigned long long best = 0ull;                                           // every key of a reached group is above 0
  for (int s = t; s < N; s += 256) {
    const int ge = roc_group_end(gend, s, N);
    const unsigned int g = P[ge - 1];
    const int TPg = (int)(g >> 16), FPg = (int)(g & 0xFFFFu);
    if (tp_curve) { tp_curve[s] = TPg; fp_curve[s] = FPg; }
    int first = 1;
    if (s > 0) first = gend[s - 1] <= s;                                    // the position before belongs to a group that ends here
    if (!first) continue;
    const unsigned int p = s > 0 ? P[s - 1] : 0u;                           // the point before: the group before, or point 0
    const int TPp = (int)(p >> 16), FPp = (int)(p & 0xFFFFu);
    const int tpg = TPg - TPp, fpg = FPg - FPp;
    pairs += (long long)tpg * (long long)(2 * (Nn - FPg) + fpg);
    if (tpg > 0) acc += (double)((long long)tpg * (long long)TPg) / (double)(TPg + FPg);
    if (tpg + fpg > 0) {                                                    // a group no draw reached is not an operating point
      const long long J = (long long)TPg * Nn - (long long)FPg * Pn;        // within +-2^26
      const unsigned long long key = (unsigned long long)(J + (1ll << 27)) << 32 | (unsigned long long)(0xFFFFFFFFu - (unsigned int)s);
      best = key > best ? key : best;                                       // the largest J, then the smallest position
    }
    if (Qspec > 0) {
      unsigned int nx = g;                                                  // the point after; the last group has none
      if (ge < N) nx = P[roc_group_end(gend, ge, N) - 1];
      const int FPn = (int)(nx & 0xFFFFu);
      for (int q = 0; q < Qspec; ++q) {
        const int need = s_spec[q] * Nn;
        const bool here = (Nn - FPg) * kRocBp >= need, after = ge < N && (Nn - FPn) * kRocBp >= need;
        int* o = at_spec + (b * Qspec + q) * 2;
        if (here && !after) { o[0] = TPg; o[1] = FPg; }                     // the last point that keeps the specificity
        else if (s == 0 && !here) { o[0] = 0; o[1] = 0; }                   // no group does: point 0
      }
    }
    for (int q = 0; q < Qsens; ++q) {
      const int need = s_sens[q] * Pn;
      const bool before = TPp * kRocBp >= need, here = TPg * kRocBp >= need;
      int* o = at_sens + (b * Qsens + q) * 2;
      if (s == 0 && before) { o[0] = 0; o[1] = 0; }                         // point 0 reaches it (level 0, or no positive row)
      else if (here && !before) { o[0] = TPg; o[1] = FPg; }                 // the first point that reaches the sensitivity
    }
  }
  acc = wave_sum(acc);
  pairs = wave_sum(pairs);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) { s_red[wave] = acc; s_auc[wave] = pairs; s_key[wave] = best; }
  __syncthreads();
  if (t < Qcut) {
    int m = cut_rows[t];
    m = m < 0 ? 0 : (m > N ? N : m);
    const unsigned int c = m > 0 ? P[m - 1] : 0u;
    at_cut[(b * Qcut + t) * 2] = (int)(c >> 16);
    at_cut[(b * Qcut + t) * 2 + 1] = (int)(c & 0xFFFFu);
  }
  if (t == 0) {
    const double sum = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    ap[b] = Pn > 0 ? sum / (double)Pn : __builtin_nan("");
    auc2[b] = ((s_auc[0] + s_auc[1]) + s_auc[2]) + s_auc[3];
    total[b * 2] = Pn;
    total[b * 2 + 1] = Nn;
    unsigned long long k = s_key[0];
    for (int i = 1; i < 4; ++i) k = s_key[i] > k ? s_key[i] : k;
    const int sg = clamp_row((int)(0xFFFFFFFFu - (unsigned int)(k & 0xFFFFFFFFull)), N);   // some group is always reached: N draws
    const unsigned int y = P[roc_group_end(gend, sg, N) - 1];
    youden[b * 3] = (int)(y >> 16);
    youden[b * 3 + 1] = (int)(y & 0xFFFFu);
    youden[b * 3 + 2] = sg;
  }
}

}  // namespace gvk

extern "C" int gvk_roc_replicates(const void* strata, const int32_t* positive, const int32_t* order, const int32_t* gend,
                                  const int32_t* class_rows, const int32_t* class_off, const int32_t* spec_bp, const int32_t* sens_bp,
                                  const int32_t* cut_rows, int32_t* total, int64_t* auc2, double* ap, int32_t* at_spec, int32_t* at_sens,
                                  int32_t* at_cut, int32_t* youden, int32_t* tp, int32_t* fp, int N, int K, int Qspec, int Qsens, int Qcut, int R,
                                  uint64_t seed, int stratified, int resample, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(positive && order && gend && total && auc2 && ap && youden, "gvk_roc_replicates: bad arguments");
  GVK_REQUIRE(N >= 1 && N <= kRocMaxN, "gvk_roc_replicates: N = %d rows outside [1, %d] (one workgroup keeps the multiplicities and the scan in LDS)", N,
              kRocMaxN);
  GVK_REQUIRE(Qspec >= 0 && Qspec <= kRocMaxQ && Qsens >= 0 && Qsens <= kRocMaxQ && Qcut >= 0 && Qcut <= kRocMaxQ,
              "gvk_roc_replicates: (%d, %d, %d) specificity / sensitivity / cut levels, each list outside [0, %d]", Qspec, Qsens, Qcut, kRocMaxQ);
  GVK_REQUIRE(Qspec == 0 || (spec_bp && at_spec), "gvk_roc_replicates: Qspec = %d needs the spec_bp and at_spec arrays", Qspec);
  GVK_REQUIRE(Qsens == 0 || (sens_bp && at_sens), "gvk_roc_replicates: Qsens = %d needs the sens_bp and at_sens arrays", Qsens);
  GVK_REQUIRE(Qcut == 0 || (cut_rows && at_cut), "gvk_roc_replicates: Qcut = %d needs the cut_rows and at_cut arrays", Qcut);
  GVK_REQUIRE(R >= 1, "gvk_roc_replicates: R = %d replicates (at least 1)", R);
  GVK_REQUIRE(resample == 0 || resample == 1, "gvk_roc_replicates: resample = %d (0 or 1)", resample);
  GVK_REQUIRE(stratified == 0 || stratified == 1, "gvk_roc_replicates: stratified = %d (0 or 1)", stratified);
  GVK_REQUIRE(resample || R == 1, "gvk_roc_replicates: resample = 0 is the full sample, R = %d must be 1", R);
  GVK_REQUIRE(!(resample && stratified) || (strata && class_rows && class_off && K >= 1 && K <= kRocMaxK),
              "gvk_roc_replicates: the stratified rule needs strata, class_rows, class_off and 1 <= K <= %d (K = %d)", kRocMaxK, K);
  GVK_REQUIRE((tp == nullptr) == (fp == nullptr), "gvk_roc_replicates: tp and fp come together");
  GVK_REQUIRE(!resample || !tp, "gvk_roc_replicates: the curve (tp, fp) is written with resample = 0 only");
  const int Npad = scan_pad(N);
  const size_t lds = sizeof(unsigned int) * (size_t)2 * Npad;
  static size_t granted = 64 * 1024 - 256;                                  // what a launch may ask for without the attribute (the static arrays take a little)
  if (int rc = ensure_lds(&roc_replicates_kernel, lds, granted, "roc_replicates")) return rc;
  GVK_LAUNCH(roc_replicates_kernel, dim3((unsigned)R), dim3(256), (unsigned)lds, (hipStream_t)stream, (const long long*)strata,
             (const int*)positive, (const int*)order, (const int*)gend, (const int*)class_rows, (const int*)class_off, (const int*)spec_bp,
             (const int*)sens_bp, (const int*)cut_rows, (int*)total, (long long*)auc2, ap, (int*)at_spec, (int*)at_sens, (int*)at_cut,
             (int*)youden, (int*)tp, (int*)fp, N, K, Qspec, Qsens, Qcut, Npad, (unsigned long long)seed, stratified, resample);
  return check_launch("roc_replicates");
}
