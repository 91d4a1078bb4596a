// Bootstrap replicates of the evaluation metrics (gaviko_amd.metrics.bootstrap / compare): replicate b resamples the N rows of an
// evaluation set with replacement and leaves what csrc/metrics.hip leaves for the full sample -- the K x K confusion counts and the
// one-vs-rest AUC pair counts of every class -- as exact integers.  A resample is a vector of integer multiplicities w_i on the rows:
//   confusion[t][p]   = sum of w_i over the rows with (label, prediction) = (t, p)
//   2*greater + ties  = sum over positives i and negatives j of  w_i w_j (2 [p_i > p_j] + [p_i == p_j])
// With the rows of class column c sorted once per call (order, and the tie group [gstart, gend) of every sorted position), the pair sum of a
// replicate is a prefix sum: P = inclusive scan of the negatives' weights in sorted order, and a positive at sorted position s adds
//   w (2 P[gstart - 1] + (P[gend - 1] - P[gstart - 1])) = w (P[gstart - 1] + P[gend - 1]),     P[-1] = 0
// -- O(N) per class and replicate, against O(N^2) for counting pairs.  Everything is an integer: the order of the atomics changes nothing.
#include "replicate.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kBootMaxN = GVK_BOOTSTRAP_MAX_ROWS;               // multiplicities stay below 2^24 (the label shares their LDS word), two N-entry LDS arrays
constexpr int kBootMaxK = GVK_BOOTSTRAP_MAX_CLASSES;            // the label takes the 8 bits above them; K x K counters in LDS

// One 256-thread workgroup per replicate.  LDS (dynamic): wl[Npad] | P[Npad] | conf[K * K], Npad = N rounded up to the scan tile.
//   wl[row] = label << 24 | multiplicity: the label is laid down first, the N draws of the replicate add 1 each (32-bit LDS atomics; a
//   multiplicity is at most N <= 8192, so it never reaches the label), and every later pass gets both from one LDS read.
// Per class c: P[s] = weight of the row at sorted position s if it is a negative, else 0; inclusive scan of P (block_scan_tiles_u32 of
// replicate.hpp); the positives' sums; a block reduction; plain stores.  Every index read from a table is clamped or tested before it
// addresses LDS: the tables are the caller's contract (ops.bootstrap_counts builds them), a broken one gives wrong counts, never an access
// outside the arrays.
__global__ __launch_bounds__(256) void bootstrap_counts_kernel(const long long* __restrict__ labels, const int* __restrict__ pred,
                                                               const int* __restrict__ order, const int* __restrict__ gstart,
                                                               const int* __restrict__ gend, const int* __restrict__ class_rows,
                                                               const int* __restrict__ class_off, long long* __restrict__ confusion,
                                                               long long* __restrict__ auc_counts, int N, int K, int Npad,
                                                               unsigned long long seed, int stratified) {
  extern __shared__ __attribute__((aligned(16))) unsigned int boot_lds[];
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned long long s_red[8];
  unsigned int* wl = boot_lds;
  unsigned int* P = boot_lds + Npad;
  unsigned int* conf = boot_lds + 2 * Npad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long b = blockIdx.x;

  for (int i = t; i < N; i += 256) {
    const long long y = labels[i];
    wl[i] = (y >= 0 && y < K) ? (unsigned int)y << 24 : 0xFF000000u;      // a label outside [0, K) (the caller rejects it) matches no class
  }
  for (int i = t; i < K * K; i += 256) conf[i] = 0u;
  __syncthreads();
  for (int n = t; n < N; n += 256) atomicAdd(&wl[draw_row(seed, b, n, N, K, labels, class_rows, class_off, stratified)], 1u);
  __syncthreads();
  for (int i = t; i < N; i += 256) {
    const unsigned int v = wl[i], y = v >> 24, w = v & 0xFFFFFFu;
    const int p = pred[i];
    if (w && y < (unsigned int)K && p >= 0 && p < K) atomicAdd(&conf[y * K + p], w);
  }
  __syncthreads();
  for (int i = t; i < K * K; i += 256) confusion[b * K * K + i] = (long long)conf[i];

  for (int c = 0; c < K; ++c) {
    const int* oc = order + (size_t)c * N;
    for (int s = t; s < Npad; s += 256) {
      unsigned int w = 0u;
      if (s < N) {
        const unsigned int v = wl[clamp_row(oc[s], N)];
        w = (v >> 24) != (unsigned int)c ? (v & 0xFFFFFFu) : 0u;
      }
      P[s] = w;
    }
    __syncthreads();
    const unsigned int carry = block_scan_tiles_u32(P, Npad, s_wave);
    unsigned long long acc = 0ull, npos = 0ull;
    for (int s = t; s < N; s += 256) {
      const unsigned int v = wl[clamp_row(oc[s], N)], w = v & 0xFFFFFFu;
      if ((v >> 24) == (unsigned int)c && w) {
        int gs = gstart[(size_t)c * N + s], ge = gend[(size_t)c * N + s];
        gs = gs < 0 ? 0 : (gs > N ? N : gs);
        ge = ge < 1 ? 1 : (ge > N ? N : ge);
        const unsigned int below = gs > 0 ? P[gs - 1] : 0u;               // negatives' weight strictly below the tie group
        acc += (unsigned long long)w * ((unsigned long long)below + (unsigned long long)P[ge - 1]);
        npos += w;
      }
    }
    acc = wave_sum(acc);
    npos = wave_sum(npos);
    if (lane == 0) { s_red[wave] = acc; s_red[4 + wave] = npos; }
    __syncthreads();
    if (t == 0) {
      const unsigned long long a = s_red[0] + s_red[1] + s_red[2] + s_red[3], np = s_red[4] + s_red[5] + s_red[6] + s_red[7];
      long long* out = auc_counts + (b * K + c) * 3;
      out[0] = (long long)a;
      out[1] = (long long)np;
      out[2] = (long long)carry;                                          // the scan's total: the negatives' weight
    }
    __syncthreads();                                                      // P and s_red are rewritten by the next class
  }
}

}  // namespace gvk

extern "C" int gvk_bootstrap_counts(const void* labels, const int32_t* pred, const int32_t* order, const int32_t* gstart, const int32_t* gend,
                                    const int32_t* class_rows, const int32_t* class_off, int64_t* confusion, int64_t* auc_counts, int N, int K, int R,
                                    uint64_t seed, int stratified, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(labels && pred && order && gstart && gend && confusion && auc_counts, "gvk_bootstrap_counts: bad arguments");
  GVK_REQUIRE(N >= 1 && N <= kBootMaxN, "gvk_bootstrap_counts: N = %d rows outside [1, %d] (one workgroup keeps the multiplicities and the scan in LDS)", N,
              kBootMaxN);
  GVK_REQUIRE(K >= 2 && K <= kBootMaxK, "gvk_bootstrap_counts: K = %d classes outside [2, %d]", K, kBootMaxK);
  GVK_REQUIRE(R >= 1, "gvk_bootstrap_counts: R = %d replicates (at least 1)", R);
  GVK_REQUIRE(stratified == 0 || stratified == 1, "gvk_bootstrap_counts: stratified = %d (0 or 1)", stratified);
  GVK_REQUIRE(!stratified || (class_rows && class_off), "gvk_bootstrap_counts: the stratified rule needs class_rows and class_off");
  const int Npad = scan_pad(N);
  const size_t lds = sizeof(unsigned int) * ((size_t)2 * Npad + (size_t)K * K);
  static size_t granted = 64 * 1024 - 256;                                // what a launch may ask for without the attribute (the static arrays take a little)
  if (int rc = ensure_lds(&bootstrap_counts_kernel, lds, granted, "bootstrap_counts")) return rc;
  GVK_LAUNCH(bootstrap_counts_kernel, dim3((unsigned)R), dim3(256), (unsigned)lds, (hipStream_t)stream, (const long long*)labels, (const int*)pred,
             (const int*)order, (const int*)gstart, (const int*)gend, (const int*)class_rows, (const int*)class_off, (long long*)confusion,
             (long long*)auc_counts, N, K, Npad, (unsigned long long)seed, stratified);
  return check_launch("bootstrap_counts");
}
