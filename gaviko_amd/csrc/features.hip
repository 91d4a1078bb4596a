// Feature embeddings and kNN probes (gaviko_amd.features): what a user of the reference gets from a forward pre-hook on the head's
// nn.Linear, a hook per block, and sklearn's NearestNeighbors / NearestCentroid on the host.  Everything here is fp32, uses no atomics and
// sums in a fixed order: two runs are bit-identical.
//   token_pool         out[b][c] = mean over the rows [r0, r0 + R) of a token stream [B][T][C]        (per-layer CLS row / patch mean)
//   l2_normalize_rows  y[n] = x[n] / max(||x[n]||, eps)                                                (cosine = normalise + inner product)
//   feature_topk       the k best bank rows of every query, inner product or squared L2, exact (score, index) order
//   knn_vote           neighbour lists + bank labels -> class probabilities and the prediction
//   class_means        per-class mean rows (prototypes) and counts
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// ---------------------------------------------------------------------------------------------------------------- token_pool
// One workgroup of 16 waves per (64-column tile, sample).  Wave w adds the rows r0 + w, r0 + w + 16, ... in that order (lane = column, 256
// contiguous bytes per row and wave, four loads in flight); the 16 partial rows meet in LDS and are added as a fixed binary tree.  The order
// depends on R alone: not on B, not on the grid.  R = 1: wave 0 holds the row, the other partials are never formed -- the row is copied.
// Algorithmic bytes: B * R * C * 4 read, B * C * 4 written.
constexpr int kPoolWaves = 16;

__global__ __launch_bounds__(64 * kPoolWaves) void token_pool_kernel(const float* __restrict__ g, float* __restrict__ out, int T, int C, int r0, int R) {
  __shared__ float part[kPoolWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
  const bool live = c < C;
  const float* base = g + ((int64_t)b * T + r0) * C + (live ? c : 0);
  if (R == 1) {
    if (w == 0 && live) out[(int64_t)b * C + c] = base[0];
    return;
  }
  float s = 0.f;
  int r = w;
  for (; r + 3 * kPoolWaves < R; r += 4 * kPoolWaves) {
    const float v0 = base[(int64_t)r * C], v1 = base[(int64_t)(r + kPoolWaves) * C], v2 = base[(int64_t)(r + 2 * kPoolWaves) * C],
                v3 = base[(int64_t)(r + 3 * kPoolWaves) * C];
    s += v0;
    s += v1;
    s += v2;
    s += v3;
  }
  for (; r < R; r += kPoolWaves) s += base[(int64_t)r * C];
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && live) {
    float t[kPoolWaves];
#pragma unroll
    for (int i = 0; i < kPoolWaves; ++i) t[i] = part[i][lane];
#pragma unroll
    for (int n = kPoolWaves / 2; n > 0; n >>= 1)
#pragma unroll
      for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    out[(int64_t)b * C + c] = t[0] / (float)R;
  }
}

// ---------------------------------------------------------------------------------------------------------------- l2_normalize_rows
// One wave per row: lane l squares and adds the columns l, l + 64, ... in that order, the 64 partials meet in the xor butterfly (the same
// bits in every lane).  The row is read again for the division, element by element by the lane that writes it: in place is safe.
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ norm, int N, int C,
                                                           float eps) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;                                           // uniform over the wave
  const float* xr = x + (int64_t)n * C;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) ss += xr[c] * xr[c];
  ss = wave_sum(ss);
  const float nr = sqrtf(ss), den = fmaxf(nr, eps);
  float* yr = y + (int64_t)n * C;
  for (int c = lane; c < C; c += 64) yr[c] = xr[c] / den;
  if (norm && lane == 0) norm[n] = nr;
}

// ---------------------------------------------------------------------------------------------------------------- feature_topk
// Ordering of candidates: a larger key is better, an equal key goes to the lower bank index.  key = score (inner product) or -distance
// (squared L2; the negation is exact), so one rule serves both metrics.  The sentinel (-inf, INT_MAX) loses to every real candidate.
constexpr int kTopkMaxK = 32;
constexpr int kTopkWaves = 4;
constexpr int kTopkMaxSlabs = 128;
constexpr int kListPitch = kTopkMaxK + 1;                       // 33: the 16 lanes that walk 16 lists fall on 16 banks

__device__ __forceinline__ bool better(float k1, int i1, float k2, int i2) { return k1 > k2 || (k1 == k2 && i1 < i2); }
__device__ __forceinline__ bool better3(float k1, int i1, int w1, float k2, int i2, int w2) {
  return k1 > k2 || (k1 == k2 && (i1 < i2 || (i1 == i2 && w1 < w2)));
}

// One wave merges P sorted lists (best first, k entries each, list p at lk / li + p * pstride) into the k best, written by lane 0 to
// ok / oi.  Lane l owns the lists l, l + 64, ... (PL of them) and a head position in each; every step is one butterfly for the best head
// under the (key, index, list) order and one advance.  The order is total, so the result does not depend on how the candidates were cut into
// lists.  negate: write -key (the squared-L2 distance).  An exhausted output slot (fewer than k real candidates: NaN scores) gets index -1.
template <int PL, typename KP, typename IP>
__device__ __forceinline__ void wave_merge(KP lk, IP li, int P, int pstride, int k, int lane, float* ok, int* oi, bool negate) {
  int h[PL];
#pragma unroll
  for (int m = 0; m < PL; ++m) h[m] = 0;
  for (int j = 0; j < k; ++j) {
    float bk = -INFINITY;
    int bi = INT_MAX, bw = INT_MAX;
#pragma unroll
    for (int m = 0; m < PL; ++m) {
      const int p = lane + 64 * m;
      if (p < P && h[m] < k) {
        const float ck = lk[p * pstride + h[m]];
        const int ci = li[p * pstride + h[m]];
        if (better3(ck, ci, p, bk, bi, bw)) { bk = ck; bi = ci; bw = p; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float k2 = __shfl_xor(bk, o, 64);
      const int i2 = __shfl_xor(bi, o, 64), w2 = __shfl_xor(bw, o, 64);
      if (better3(k2, i2, w2, bk, bi, bw)) { bk = k2; bi = i2; bw = w2; }
    }
#pragma unroll
    for (int m = 0; m < PL; ++m)
      if (lane + 64 * m == bw) h[m] += 1;
    if (lane == 0) {
      ok[j] = negate ? -bk : bk;
      oi[j] = bi == INT_MAX ? -1 : bi;
    }
  }
}

// sum of squares of the columns a lane holds of its row, in super-step order, then over the four lanes of the row: depends on C alone
__device__ __forceinline__ float sq4(f32x4 v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }

// Workgroup = (16-query tile, bank slab), four waves.  The query tile sits in LDS (row pitch Cp + 4 floats, columns C.. zero).  Wave w takes
// the slab's 16-row bank tiles w, w + 4, ...: S[query][bank row] = Q . G^T on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32
// accumulation), the contraction in super-steps of 16 columns -- lane (r = lane & 15, kq = lane >> 4) supplies columns 16 s + 4 kq + e of
// query r (A) and of bank row r (B, one 16-byte load straight from global memory) to MFMA e -- so a score is the same chain of operations
// whatever tile, slab or call it is computed in.  The 16 x 16 scores go through LDS to the lanes 0..15, one per query, which keep that
// query's sorted top-k list (insertion under the (key, index) order; a candidate that does not beat the list's last entry costs one
// compare).  At the end the four waves' lists are merged per query (wave_merge) into the slab's list in global scratch.
template <bool L2>
__global__ __launch_bounds__(64 * kTopkWaves) void topk_slab_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                                   const int* __restrict__ exclude, float* __restrict__ pkey, int* __restrict__ pidx,
                                                                   int Nq, int Ng, int C, int k, int nslabs, int tps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nss = (C + 15) >> 4, Cp = nss * 16, pitch = Cp + 4;
  float* sQ = smem;                                             // [16][pitch]
  float* sT = sQ + 16 * pitch;                                  // [waves][16][17] score tiles
  float* sK = sT + kTopkWaves * 16 * 17;                        // [waves][16][33] list keys
  int* sI = (int*)(sK + kTopkWaves * 16 * kListPitch);          // [waves][16][33] list indices
  float* sN = (float*)(sI + kTopkWaves * 16 * kListPitch);      // [16] query norms
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int q0 = blockIdx.x * 16, slab = blockIdx.y;
  // ---- the query tile (rows past Nq repeat the last row; their results are never written)
  const int c4n = Cp >> 2;
  for (int i = tid; i < 16 * c4n; i += 64 * kTopkWaves) {
    const int row = i / c4n, c4 = i - row * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (4 * c4 < C) v = *(const f32x4*)(q + (int64_t)min(q0 + row, Nq - 1) * C + 4 * c4);
    *(f32x4*)(sQ + row * pitch + 4 * c4) = v;
  }
  float* lk = sK + w * 16 * kListPitch;
  int* li = sI + w * 16 * kListPitch;
  for (int i = lane; i < 16 * kListPitch; i += 64) { lk[i] = -INFINITY; li[i] = INT_MAX; }
  __syncthreads();
  if (L2 && w == 0) {
    float s = 0.f;
    for (int ss = 0; ss < nss; ++ss) s += sq4(*(const f32x4*)(sQ + r * pitch + 16 * ss + 4 * kq));
    s = kq_sum(s);
    if (kq == 0) sN[r] = s;
  }
  if (L2) __syncthreads();
  // ---- this wave's bank tiles
  const int ntiles = (Ng + 15) >> 4;
  const int t0 = slab * tps, t1 = min(t0 + tps, ntiles);
  const int nfull = C >> 4;
  float* tile = sT + w * 16 * 17;
  const int myq = q0 + lane;                                    // lanes 0..15: the query whose list the lane keeps
  const int excl = (lane < 16 && exclude && myq < Nq) ? exclude[myq] : -1;
  int nlist = 0;
  float wk = -INFINITY;                                         // the list's last entry once it is full
  int wi = INT_MAX;
  const float* arow = sQ + r * pitch + 4 * kq;
  for (int t = t0 + w; t < t1; t += kTopkWaves) {
    const int g0 = t * 16;
    const float* brow = g + (int64_t)min(g0 + r, Ng - 1) * C + 4 * kq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float gn = 0.f;
#pragma unroll 4
    for (int ss = 0; ss < nfull; ++ss) {
      const f32x4 b4 = *(const f32x4*)(brow + 16 * ss);
      const f32x4 a4 = *(const f32x4*)(arow + 16 * ss);
      acc = mfma4(a4.x, b4.x, acc);
      acc = mfma4(a4.y, b4.y, acc);
      acc = mfma4(a4.z, b4.z, acc);
      acc = mfma4(a4.w, b4.w, acc);
      if (L2) gn += sq4(b4);
    }
    if (nfull < nss) {                                          // C % 16 != 0: the columns past C are zero on both sides
      f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
      if (16 * nfull + 4 * kq < C) b4 = *(const f32x4*)(brow + 16 * nfull);
      const f32x4 a4 = *(const f32x4*)(arow + 16 * nfull);
      acc = mfma4(a4.x, b4.x, acc);
      acc = mfma4(a4.y, b4.y, acc);
      acc = mfma4(a4.z, b4.z, acc);
      acc = mfma4(a4.w, b4.w, acc);
      if (L2) gn += sq4(b4);
    }
    if (L2) gn = kq_sum(gn);                                    // ||g[g0 + r]||^2, r = lane & 15 = this lane's score column
    // accumulator: lane holds S[query 4 kq + e][bank row r]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qi = 4 * kq + e;
      const float s = acc[e];
      tile[qi * 17 + r] = L2 ? -((sN[qi] + gn) - 2.f * s) : s;
    }
    wave_lds_sync();
    if (lane < 16) {
      for (int j = 0; j < 16; ++j) {
        const int idx = g0 + j;
        const float ck = tile[lane * 17 + j];
        if (idx >= Ng || idx == excl || !(ck == ck)) continue;
        if (nlist == k && !better(ck, idx, wk, wi)) continue;
        int p = nlist < k ? nlist : k - 1;
        float* mk = lk + lane * kListPitch;
        int* mi = li + lane * kListPitch;
        while (p > 0 && better(ck, idx, mk[p - 1], mi[p - 1])) {
          mk[p] = mk[p - 1];
          mi[p] = mi[p - 1];
          --p;
        }
        mk[p] = ck;
        mi[p] = idx;
        if (nlist < k) ++nlist;
        if (nlist == k) { wk = mk[k - 1]; wi = mi[k - 1]; }
      }
    }
    wave_lds_sync();
  }
  __syncthreads();
  // ---- the four waves' lists of a query -> the slab's list.  list p = wave p's: sK + p * 16 * 33 + query * 33
  for (int qi = w; qi < 16; qi += kTopkWaves) {
    const int qq = q0 + qi;
    if (qq >= Nq) break;                                        // uniform over the wave
    const int64_t o = ((int64_t)qq * nslabs + slab) * k;
    wave_merge<1>(sK + qi * kListPitch, sI + qi * kListPitch, kTopkWaves, 16 * kListPitch, k, lane, pkey + o, pidx + o, false);
  }
}

// One wave per query: the slab lists (sorted, in global scratch) are staged in LDS and merged by the same rule.
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ pkey, const int* __restrict__ pidx, float* __restrict__ score,
                                                        int* __restrict__ idx, int k, int nslabs, int negate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sk = smem;
  int* si = (int*)(smem + nslabs * k);
  const int qq = blockIdx.x, lane = threadIdx.x;
  const int64_t base = (int64_t)qq * nslabs * k;
  for (int i = lane; i < nslabs * k; i += 64) { sk[i] = pkey[base + i]; si[i] = pidx[base + i]; }
  __syncthreads();
  wave_merge<kTopkMaxSlabs / 64>(sk, si, nslabs, k, k, lane, score + (int64_t)qq * k, idx + (int64_t)qq * k, negate != 0);
}

// ---------------------------------------------------------------------------------------------------------------- knn_vote
// One wave per query, lane l holds the classes l, l + 64, l + 128, l + 192.  The k neighbours are walked in rank order; weight and sums
// are kept in double (k <= 32 terms: free), so the only fp32 rounding is the final store.  mode 0: weight 1, probs = count / k.
// mode 1: w_j = exp((score_j - score_0) / T), probs = sum / total.  A neighbour index outside [0, Ng) (the -1 of an unfilled slot) or a
// label outside [0, K) has no vote.  pred = the lowest class with the largest sum.
constexpr int kVoteKPL = 4;

__global__ __launch_bounds__(256) void knn_vote_kernel(const int* __restrict__ idx, const float* __restrict__ score, const int* __restrict__ labels,
                                                       float* __restrict__ probs, int* __restrict__ pred, int Nq, int Ng, int k, int K, int mode,
                                                       float temperature) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= Nq) return;                                          // uniform over the wave
  double acc[kVoteKPL];
#pragma unroll
  for (int m = 0; m < kVoteKPL; ++m) acc[m] = 0.0;
  double total = 0.0;
  const double s0 = (double)score[(int64_t)n * k], T = (double)temperature;
  for (int j = 0; j < k; ++j) {
    const int id = idx[(int64_t)n * k + j];
    const double wj = mode == 0 ? 1.0 : exp(((double)score[(int64_t)n * k + j] - s0) / T);
    const int lbl = (id >= 0 && id < Ng) ? labels[id] : -1;
    if (lbl < 0 || lbl >= K) continue;
    total += wj;
#pragma unroll
    for (int m = 0; m < kVoteKPL; ++m) acc[m] += (lbl == lane + 64 * m) ? wj : 0.0;
  }
  const double den = mode == 0 ? (double)k : total;
  double top = -1.0;
  int am = INT_MAX;
#pragma unroll
  for (int m = 0; m < kVoteKPL; ++m) {
    const int c = lane + 64 * m;
    if (c < K) {
      const double p = den > 0.0 ? acc[m] / den : 0.0;
      probs[(int64_t)n * K + c] = (float)p;
      if (p > top) { top = p; am = c; }                         // ascending classes per lane: the lowest of equal ones stays
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t2 = __shfl_xor(top, o, 64);
    const int a2 = __shfl_xor(am, o, 64);
    if (t2 > top || (t2 == top && a2 < am)) { top = t2; am = a2; }
  }
  if (lane == 0) pred[n] = am < K ? am : 0;
}

// ---------------------------------------------------------------------------------------------------------------- class_means
// One workgroup per (class, 256-column tile); a thread owns one column and walks all N rows in row order, adding the rows of its class.
// N is a dataset (hundreds to thousands of rows), not a token stream.  An empty class: count 0 and exact zeros.
__global__ __launch_bounds__(256) void class_means_kernel(const float* __restrict__ x, const int* __restrict__ labels, float* __restrict__ mean,
                                                          int* __restrict__ count, int N, int C) {
  const int cls = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  const bool live = c < C;
  float s = 0.f;
  int cnt = 0;
  for (int n = 0; n < N; ++n) {
    if (labels[n] == cls) {                                     // uniform over the workgroup
      cnt += 1;
      if (live) s += x[(int64_t)n * C + c];
    }
  }
  if (live) mean[(int64_t)cls * C + c] = cnt > 0 ? s / (float)cnt : 0.f;
  if (blockIdx.y == 0 && threadIdx.x == 0) count[cls] = cnt;
}

static int topk_slabs(int Nq, int Ng, int want) {
  const int ntiles = (Ng + 15) / 16, nqt = (Nq + 15) / 16;
  int n;
  if (want > 0) {
    n = want;
  } else {
    n = 1024 / nqt;                                             // about four workgroups per CU over the whole grid
    const int per_wave = (ntiles + kTopkWaves - 1) / kTopkWaves;   // at least one bank tile per wave
    n = n < per_wave ? n : per_wave;
  }
  n = n < 1 ? 1 : (n > kTopkMaxSlabs ? kTopkMaxSlabs : n);
  n = n > ntiles ? ntiles : n;
  const int tps = (ntiles + n - 1) / n;
  return (ntiles + tps - 1) / tps;                              // no empty slab
}

}  // namespace gvk

extern "C" int gvk_token_pool(const float* g, float* out, int B, int T, int C, int r0, int R, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(g && out && B > 0 && T > 0, "gvk_token_pool: bad arguments");
  GVK_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, "gvk_token_pool: C = %d (a multiple of 4 within [4, 1024])", C);
  GVK_REQUIRE(r0 >= 0 && R >= 1 && R <= T - r0, "gvk_token_pool: rows [%d, %d + %d) outside the %d rows of the stream", r0, r0, R, T);
  GVK_REQUIRE(B <= 65535, "gvk_token_pool: B = %d samples per launch (at most 65535)", B);
  GVK_LAUNCH(token_pool_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(64 * kPoolWaves), 0, (hipStream_t)stream, g, out, T, C, r0, R);
  return check_launch("token_pool");
}

extern "C" int gvk_l2_normalize_rows(const float* x, float* y, float* norm, int N, int C, float eps, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && y && N > 0 && C > 0, "gvk_l2_normalize_rows: bad arguments");
  GVK_REQUIRE(eps > 0.f, "gvk_l2_normalize_rows: eps = %g (must be positive)", (double)eps);
  GVK_REQUIRE(x == y || y + (int64_t)N * C <= x || x + (int64_t)N * C <= y, "gvk_l2_normalize_rows: y must be x itself or not overlap it");
  GVK_LAUNCH(l2_normalize_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, norm, N, C, eps);
  return check_launch("l2_normalize_rows");
}

extern "C" int gvk_feature_topk_slabs(int Nq, int Ng, int want) {
  if (Nq < 1 || Ng < 1) return 0;
  return gvk::topk_slabs(Nq, Ng, want);
}

extern "C" int gvk_feature_topk(const gvk_feature_topk_desc* d, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(d && d->q && d->g && d->idx && d->score && d->scratch, "gvk_feature_topk: bad arguments");
  const int Nq = d->Nq, Ng = d->Ng, C = d->C, k = d->k;
  GVK_REQUIRE(Nq >= 1 && Ng >= 1, "gvk_feature_topk: Nq = %d, Ng = %d (at least 1 each)", Nq, Ng);
  GVK_REQUIRE((int64_t)Nq * Ng < (1LL << 31), "gvk_feature_topk: Nq * Ng = %lld exceeds the 32-bit range", (long long)Nq * Ng);
  GVK_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, "gvk_feature_topk: C = %d (a multiple of 4 within [4, 1024])", C);
  GVK_REQUIRE(d->metric == 0 || d->metric == 1, "gvk_feature_topk: metric = %d (0 inner product, 1 squared L2)", d->metric);
  const int avail = Ng - (d->exclude ? 1 : 0);
  GVK_REQUIRE(k >= 1 && k <= kTopkMaxK && k <= avail, "gvk_feature_topk: k = %d outside [1, min(%d, %d)]", k, kTopkMaxK, avail);
  const int nslabs = d->nslabs;
  GVK_REQUIRE(nslabs >= 1 && nslabs == topk_slabs(Nq, Ng, nslabs), "gvk_feature_topk: nslabs = %d is not a count gvk_feature_topk_slabs returns for this shape",
              nslabs);
  const int ntiles = (Ng + 15) / 16, tps = (ntiles + nslabs - 1) / nslabs;
  const int64_t words = (int64_t)Nq * nslabs * k;
  GVK_REQUIRE(d->scratch_words >= 2 * words, "gvk_feature_topk: scratch of %lld words, %lld needed", (long long)d->scratch_words, (long long)(2 * words));
  float* pkey = (float*)d->scratch;
  int* pidx = (int*)d->scratch + words;
  const int Cp = ((C + 15) / 16) * 16;
  const size_t lds = (size_t)(16 * (Cp + 4) + kTopkWaves * 16 * 17 + 2 * kTopkWaves * 16 * kListPitch + 16) * sizeof(float);
  const dim3 grid((unsigned)((Nq + 15) / 16), (unsigned)nslabs), block(64 * kTopkWaves);
  static size_t granted_ip = 64 * 1024, granted_l2 = 64 * 1024;
  if (d->metric == 1) {
    if (int rc = ensure_lds(&topk_slab_kernel<true>, lds, granted_l2, "topk_slab<l2>")) return rc;
    GVK_LAUNCH(topk_slab_kernel<true>, grid, block, (unsigned)lds, (hipStream_t)stream, (const float*)d->q, (const float*)d->g, (const int*)d->exclude,
               pkey, pidx, Nq, Ng, C, k, nslabs, tps);
  } else {
    if (int rc = ensure_lds(&topk_slab_kernel<false>, lds, granted_ip, "topk_slab<ip>")) return rc;
    GVK_LAUNCH(topk_slab_kernel<false>, grid, block, (unsigned)lds, (hipStream_t)stream, (const float*)d->q, (const float*)d->g, (const int*)d->exclude,
               pkey, pidx, Nq, Ng, C, k, nslabs, tps);
  }
  GVK_LAUNCH(topk_merge_kernel, dim3((unsigned)Nq), dim3(64), (unsigned)(2 * nslabs * k * sizeof(float)), (hipStream_t)stream, (const float*)pkey,
             (const int*)pidx, (float*)d->score, (int*)d->idx, k, nslabs, d->metric);
  return check_launch("feature_topk");
}

extern "C" int gvk_knn_vote(const int32_t* idx, const float* score, const int32_t* labels, float* probs, int32_t* pred, int Nq, int Ng, int k, int K,
                            int mode, float temperature, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(idx && score && labels && probs && pred && Nq > 0 && Ng > 0, "gvk_knn_vote: bad arguments");
  GVK_REQUIRE(k >= 1 && k <= kTopkMaxK, "gvk_knn_vote: k = %d outside [1, %d]", k, kTopkMaxK);
  GVK_REQUIRE(K >= 2 && K <= 64 * kVoteKPL, "gvk_knn_vote: K = %d classes outside [2, %d]", K, 64 * kVoteKPL);
  GVK_REQUIRE(mode == 0 || mode == 1, "gvk_knn_vote: mode = %d (0 uniform, 1 softmax weights)", mode);
  GVK_REQUIRE(mode == 0 || temperature > 0.f, "gvk_knn_vote: temperature = %g (must be positive)", (double)temperature);
  GVK_LAUNCH(knn_vote_kernel, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const int*)idx, score, (const int*)labels, probs,
             (int*)pred, Nq, Ng, k, K, mode, temperature);
  return check_launch("knn_vote");
}

extern "C" int gvk_class_means(const float* x, const int32_t* labels, float* mean, int32_t* count, int N, int C, int K, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && labels && mean && count && N > 0 && C > 0, "gvk_class_means: bad arguments");
  GVK_REQUIRE(K >= 1 && K <= 65535, "gvk_class_means: K = %d classes outside [1, 65535]", K);
  GVK_LAUNCH(class_means_kernel, dim3((unsigned)K, (unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (const int*)labels, mean,
             (int*)count, N, C);
  return check_launch("class_means");
}
