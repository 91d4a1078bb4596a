// Out-of-distribution statistics (gaviko_amd.ood): what a user of the reference gets from numpy / sklearn.covariance on features copied to
// the host.  fp32 in, no atomics, every sum in a fixed order: two runs are bit-identical.
//   scatter_matrix   S = sum_i d_i d_i^T (f64, not divided), r4 = sum_i (||d_i||^2)^2, class counts;  d_i = fl32(x_i - mean[label_i])
//   mahalanobis      d2[n][k] = || W q_n - W m_k ||^2 for a dense whitening matrix W, the whitened rows never leaving the chip
//   logit_scores     max softmax probability, max logit, T logsumexp(z / T), softmax entropy of a row of logits
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// ---------------------------------------------------------------------------------------------------------------- scatter_matrix
// S is cut into 64 x 64 tiles; only the pairs (ta <= tb) are computed, pair p counting (0,0), (0,1), .., (0,nt-1), (1,1), ...  The rows are
// cut into chunks of kScatChunk = 64 rows at ABSOLUTE row indices (chunk c = rows [64 c, 64 c + 64)), and the chunks into `nslabs` slabs of
// `cps` consecutive chunks.  Workgroup = (pair, slab), four waves: a chunk's centred rows -- the 64 columns of tile ta and, off the diagonal,
// of tile tb -- are staged in LDS (rows past N, rows with a label outside [0, K) and columns past C as zeros); wave w owns the 16 x 64 strip
// of rows 16 w .. 16 w + 15 of the tile: four 16 x 16 accumulators on v_mfma_f32_16x16x4_f32, the contraction over the chunk's rows in row
// order (exact fp32 products, fp32 accumulation, one chain of 64 fmas per entry).  After every chunk the fp32 accumulators are added to
// double ones and cleared, so an entry of S is  sum over chunks in order of double(fp32 chain over the chunk's rows).  The slab's 64 x 64
// doubles go to scratch; scatter_finish adds the slabs in slab order and writes S[a][b] and, off the diagonal, S[b][a] from the same
// double: S equals its transpose bit for bit (inside a diagonal tile (a, b) and (b, a) are the same chain: the products commute).
// LDS: pitch 80 floats (80 mod 32 = 16): the two 16-lane row groups a 32-lane ds_read_b32 group covers fall on disjoint banks.
constexpr int kScatTile = 64;
constexpr int kScatChunk = 64;
constexpr int kScatPitch = 80;
constexpr int kScatTarget = 512;                                // workgroups wanted: two per CU

__host__ __device__ inline void scat_pair(int p, int nt, int& ta, int& tb) {
  ta = 0;
  while (p >= nt - ta) { p -= nt - ta; ++ta; }
  tb = ta + p;
}

// the split: a function of (N, C) alone (ops.scatter_split restates it for the scratch size)
static void scat_split(int N, int C, int& nt, int& npairs, int& nchunks, int& cps, int& nslabs) {
  nt = (C + kScatTile - 1) / kScatTile;
  npairs = nt * (nt + 1) / 2;
  nchunks = (N + kScatChunk - 1) / kScatChunk;
  int want = (kScatTarget + npairs - 1) / npairs;
  want = want < nchunks ? want : nchunks;
  cps = (nchunks + want - 1) / want;
  nslabs = (nchunks + cps - 1) / cps;
}

__global__ __launch_bounds__(256) void scatter_tile_kernel(const float* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ mean,
                                                           double* __restrict__ part, int N, int C, int K, int nt, int cps) {
  __shared__ __attribute__((aligned(16))) float sA[kScatChunk * kScatPitch];
  __shared__ __attribute__((aligned(16))) float sB[kScatChunk * kScatPitch];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  int ta, tb;
  scat_pair((int)blockIdx.x, nt, ta, tb);
  const bool diag = ta == tb;                                   // uniform over the workgroup
  const int a0 = ta * kScatTile, b0 = tb * kScatTile;
  const int nchunks = (N + kScatChunk - 1) / kScatChunk;
  const int c0 = (int)blockIdx.y * cps, c1 = min(c0 + cps, nchunks);
  const float* sBB = diag ? sA : sB;
  const int col4 = tid & 15, rw = tid >> 4;                     // staging: 16 threads per row of 64 columns, 16 rows per pass
  double dacc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) dacc[j][e] = 0.0;
  for (int ch = c0; ch < c1; ++ch) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rw + 16 * j;
      const int64_t n = (int64_t)ch * kScatChunk + row;
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        const int lb = labels ? labels[n] : 0;
        if (lb >= 0 && lb < K) {
          const float* xr = x + n * C;
          const float* mr = mean + (int64_t)lb * C;
          const int ca = a0 + 4 * col4, cb = b0 + 4 * col4;
          if (ca < C) va = *(const f32x4*)(xr + ca) - *(const f32x4*)(mr + ca);
          if (!diag && cb < C) vb = *(const f32x4*)(xr + cb) - *(const f32x4*)(mr + cb);
        }
      }
      *(f32x4*)(sA + row * kScatPitch + 4 * col4) = va;
      if (!diag) *(f32x4*)(sB + row * kScatPitch + 4 * col4) = vb;
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < kScatChunk / 4; ++ks) {
      const int i = 4 * ks + kq;                                // MFMA: lane (r, kq) supplies row i of the chunk, column r of its 16
      const float a = sA[i * kScatPitch + 16 * w + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = mfma4(a, sBB[i * kScatPitch + 16 * j + r], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) dacc[j][e] += (double)acc[j][e];
    __syncthreads();
  }
  // accumulator: lane holds entry (row 16 w + 4 kq + e, column 16 j + r) of the tile
  double* o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kScatTile * kScatTile);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[(16 * w + 4 * kq + e) * kScatTile + 16 * j + r] = dacc[j][e];
}

// r4: one workgroup per chunk of 64 rows, wave w the rows 16 w .. 16 w + 15 in order.  ||d||^2 in fp32: lane l squares and adds its columns
// 4 l .. 4 l + 3, 4 l + 256 .., in that order, the 64 partials meet in the xor butterfly; the square of that and the sum over rows in double;
// the four waves' sums are added as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ mean,
                                                           double* __restrict__ r4part, int N, int C, int K) {
  __shared__ double sw[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double s = 0.0;
  for (int j = 0; j < 16; ++j) {
    const int64_t n = (int64_t)blockIdx.x * kScatChunk + 16 * w + j;
    if (n >= N) break;                                          // uniform over the wave
    const int lb = labels ? labels[n] : 0;
    if (lb < 0 || lb >= K) continue;
    const float* xr = x + n * C;
    const float* mr = mean + (int64_t)lb * C;
    float ss = 0.f;
    for (int c = 4 * lane; c < C; c += 256) {
      const f32x4 d = *(const f32x4*)(xr + c) - *(const f32x4*)(mr + c);
      ss += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
    ss = wave_sum(ss);
    s += (double)ss * (double)ss;
  }
  if (lane == 0) sw[w] = s;
  __syncthreads();
  if (tid == 0) r4part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// blocks [0, 16 npairs): S from the slab partials, in slab order.  block 16 npairs: r4 -- thread t adds the chunks t, t + 256, .. in order,
// the 256 sums folded in halves (t += t + 128, then t += t + 64, ..), a fixed tree.  the blocks after it: the class counts, one wave per class (integers: exact in any order).
__global__ __launch_bounds__(256) void scatter_finish_kernel(const double* __restrict__ part, const double* __restrict__ r4part,
                                                             const int* __restrict__ labels, double* __restrict__ S, double* __restrict__ r4,
                                                             int* __restrict__ count, int N, int C, int K, int nt, int npairs, int nslabs, int nchunks) {
  __shared__ double tree[256];
  const int tid = threadIdx.x, b = (int)blockIdx.x, nsb = npairs * 16;
  if (b < nsb) {
    const int p = b >> 4, idx = (b & 15) * 256 + tid, al = idx >> 6, bl = idx & 63;
    int ta, tb;
    scat_pair(p, nt, ta, tb);
    const int a = ta * kScatTile + al, c = tb * kScatTile + bl;
    if (a >= C || c >= C) return;
    double s = 0.0;
    for (int sl = 0; sl < nslabs; ++sl) s += part[((int64_t)sl * npairs + p) * (kScatTile * kScatTile) + idx];
    S[(int64_t)a * C + c] = s;
    if (ta != tb) S[(int64_t)c * C + a] = s;
  } else if (b == nsb) {
    double s = 0.0;
    for (int c = tid; c < nchunks; c += 256) s += r4part[c];
    tree[tid] = s;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {                         // a step writes tree[0, n) and reads tree[n, 2 n) of the step before: no overlap
      if (tid < n) tree[tid] += tree[tid + n];
      __syncthreads();
    }
    if (tid == 0) r4[0] = tree[0];
  } else {
    const int cls = (b - nsb - 1) * 4 + (tid >> 6), lane = tid & 63;
    if (cls >= K) return;                                       // uniform over the wave
    int cnt = 0;
    for (int n = lane; n < N; n += 64) cnt += (labels ? labels[n] : 0) == cls ? 1 : 0;
    cnt = wave_sum(cnt);
    if (lane == 0) count[cls] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------------------------- mahalanobis
// Workgroup = 16 query rows, eight waves.  The query tile sits in LDS (row pitch Cp + 4 floats, columns C.. zero), as in feature_topk.
// The output coordinates j of z = W v are walked in chunks of 16; wave w takes the chunks w, w + 8, ...  For a chunk the wave contracts, over
// the columns c in super-steps of 16 -- lane (r = lane & 15, kq = lane >> 4) supplies columns 16 s + 4 kq + e of its row to MFMA e --
//   Zq[n][j] = sum_c q[n][c] W[j][c]   (A = the query tile from LDS, B = 16 rows of W, one 16-byte load per lane straight from global memory)
//   Zm[k][j] = sum_c m[k][c] W[j][c]   (A = 16 centres per tile, KT tiles, from global memory; the same B registers)
// so a whitened coordinate of a query and of a centre is the SAME chain of fp32 fmas: q == m[k] gives a difference of exactly 0.  The Zm tile
// goes through LDS to the lanes of its column j = r; lane (r, kq) holds Zq of the queries 4 kq + e and adds (Zq - Zm[k])^2 (one subtraction,
// one product, one addition, each rounded) to its K running sums per query, chunk after chunk.  At the end the 16 lanes of a query add their
// sums in the xor butterfly (1, 2, 4, 8) and the eight waves' sums are added in wave order: the order depends on C alone, never on Nq, the
// tile or the grid.  Rows past Nq repeat the last row and are not written; centres past K repeat the last centre and are not written.
// Cost: the grid is ceil(Nq / 16) workgroups and every one of them reads all of W (from L2) and whitens the K centres again, so the kernel is
// bound by the W traffic, not by the query bytes, and leaves CUs idle below Nq of about 4096 (256 CUs x 16 rows): a scoring call, not a GEMM.
constexpr int kMahaWaves = 8;
constexpr int kMahaMaxK = 32;

template <int KT>
__global__ __launch_bounds__(64 * kMahaWaves) void mahalanobis_kernel(const float* __restrict__ q, const float* __restrict__ W,
                                                                     const float* __restrict__ m, float* __restrict__ d2, int Nq, int C, int K) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KK = 16 * KT;
  const int nss = (C + 15) >> 4, Cp = nss * 16, pitch = Cp + 4;
  float* sQ = smem;                                             // [16][pitch]
  float* sZ = sQ + 16 * pitch;                                  // [waves][KK][17] whitened centres of the wave's chunk
  float* sP = sZ + kMahaWaves * KK * 17;                        // [waves][16][KK] the waves' sums
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int q0 = (int)blockIdx.x * 16;
  const int c4n = Cp >> 2;
  for (int i = tid; i < 16 * c4n; i += 64 * kMahaWaves) {
    const int row = i / c4n, c4 = i - row * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (4 * c4 < C) v = *(const f32x4*)(q + (int64_t)min(q0 + row, Nq - 1) * C + 4 * c4);
    *(f32x4*)(sQ + row * pitch + 4 * c4) = v;
  }
  __syncthreads();
  float acc[4][KK];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[e][k] = 0.f;
  const int nfull = C >> 4;
  const bool tail_live = 16 * nfull + 4 * kq < C;
  const float* arow = sQ + r * pitch + 4 * kq;
  float* zt = sZ + w * KK * 17;
  const float* mrow[KT];
#pragma unroll
  for (int u = 0; u < KT; ++u) mrow[u] = m + (int64_t)min(16 * u + r, K - 1) * C + 4 * kq;
  for (int t = w; t < nss; t += kMahaWaves) {
    const int j0 = 16 * t;
    const float* wrow = W + (int64_t)min(j0 + r, C - 1) * C + 4 * kq;
    f32x4 zq = {0.f, 0.f, 0.f, 0.f};
    f32x4 zm[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) zm[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ss = 0; ss < nfull; ++ss) {
      const f32x4 b4 = *(const f32x4*)(wrow + 16 * ss);
      const f32x4 a4 = *(const f32x4*)(arow + 16 * ss);
      zq = mfma4(a4.x, b4.x, zq);
      zq = mfma4(a4.y, b4.y, zq);
      zq = mfma4(a4.z, b4.z, zq);
      zq = mfma4(a4.w, b4.w, zq);
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        const f32x4 c4 = *(const f32x4*)(mrow[u] + 16 * ss);
        zm[u] = mfma4(c4.x, b4.x, zm[u]);
        zm[u] = mfma4(c4.y, b4.y, zm[u]);
        zm[u] = mfma4(c4.z, b4.z, zm[u]);
        zm[u] = mfma4(c4.w, b4.w, zm[u]);
      }
    }
    if (nfull < nss) {                                          // C % 16 != 0: the columns past C are zero on every side
      f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
      if (tail_live) b4 = *(const f32x4*)(wrow + 16 * nfull);
      const f32x4 a4 = *(const f32x4*)(arow + 16 * nfull);
      zq = mfma4(a4.x, b4.x, zq);
      zq = mfma4(a4.y, b4.y, zq);
      zq = mfma4(a4.z, b4.z, zq);
      zq = mfma4(a4.w, b4.w, zq);
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
        if (tail_live) c4 = *(const f32x4*)(mrow[u] + 16 * nfull);
        zm[u] = mfma4(c4.x, b4.x, zm[u]);
        zm[u] = mfma4(c4.y, b4.y, zm[u]);
        zm[u] = mfma4(c4.z, b4.z, zm[u]);
        zm[u] = mfma4(c4.w, b4.w, zm[u]);
      }
    }
    // accumulators: lane holds Zq[query 4 kq + e][j0 + r] and Zm[centre 16 u + 4 kq + e][j0 + r]
#pragma unroll
    for (int u = 0; u < KT; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) zt[(16 * u + 4 * kq + e) * 17 + r] = zm[u][e];
    wave_lds_sync();
    const bool livej = j0 + r < C;                              // a coordinate past C (the last chunk of C % 16 != 0) adds nothing
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      const float zk = zt[k * 17 + r];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = zq[e] - zk;
        acc[e][k] += livej ? df * df : 0.f;
      }
    }
    wave_lds_sync();
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      float v = acc[e][k];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if (r == 0) sP[(w * 16 + 4 * kq + e) * KK + k] = v;
    }
  __syncthreads();
  for (int idx = tid; idx < 16 * KK; idx += 64 * kMahaWaves) {
    const int n = idx / KK, k = idx - n * KK;
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < kMahaWaves; ++ww) s += sP[(ww * 16 + n) * KK + k];
    if (q0 + n < Nq && k < K) d2[(int64_t)(q0 + n) * K + k] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- logit_scores
// One wave per row, lane l holds the classes l, l + 64, l + 128, l + 192.  Everything in double, shifted by the row maximum; the sums per lane
// in class order, then the xor butterfly; one rounding at the store.  With s_c = z_c - max, e_c = exp(s_c) and the sums taken over every
// class but the first one at the maximum (whose term is exp(0) = 1: log1p keeps a rest far below 1), R = sum e_c, S = 1 + R:
//   out[0] = 1 / S (the largest softmax probability)   out[1] = max   out[2] = max + T log1p(sum exp(s_c / T))
//   out[3] = log1p(R) - (sum e_c s_c) / S (the entropy; a class whose e_c underflows to 0 adds 0: 0 log 0 = 0).  Both terms are >= 0.
constexpr int kLogitKPL = 4;

__global__ __launch_bounds__(256) void logit_scores_kernel(const float* __restrict__ z, float* __restrict__ out, int N, int K, double T) {
  const int n = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;                                           // uniform over the wave
  const float* zr = z + (int64_t)n * K;
  double v[kLogitKPL], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kLogitKPL; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < K ? (double)zr[c] : -INFINITY;
    mx = fmax(mx, v[i]);
  }
  mx = wave_max(mx);
  int am = INT_MAX;                                             // the first class at the maximum: its term exp(0) = 1 is kept apart
#pragma unroll
  for (int i = kLogitKPL - 1; i >= 0; --i)
    if (lane + 64 * i < K && v[i] == mx) am = lane + 64 * i;
  am = wave_min(am);
  double r1 = 0.0, rt = 0.0, se = 0.0;
#pragma unroll
  for (int i = 0; i < kLogitKPL; ++i) {
    const int c = lane + 64 * i;
    if (c < K && c != am) {
      const double d = v[i] - mx, e = exp(d);
      r1 += e;
      se += e > 0.0 ? e * d : 0.0;
      rt += exp(d / T);
    }
  }
  r1 = wave_sum(r1);
  se = wave_sum(se);
  rt = wave_sum(rt);
  if (lane == 0) {
    const double s1 = 1.0 + r1;
    float* o = out + (int64_t)n * 4;
    o[0] = (float)(1.0 / s1);
    o[1] = (float)mx;
    o[2] = (float)(mx + T * log1p(rt));
    o[3] = (float)(log1p(r1) - se / s1);
  }
}

}  // namespace gvk

extern "C" int gvk_scatter_matrix(const float* x, const int32_t* labels, const float* mean, double* S, double* r4, int32_t* count, void* scratch,
                                  int64_t scratch_bytes, int N, int C, int K, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && mean && S && r4 && count && scratch, "gvk_scatter_matrix: bad arguments");
  GVK_REQUIRE(N >= 1, "gvk_scatter_matrix: N = %d (at least 1)", N);
  GVK_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, "gvk_scatter_matrix: C = %d (a multiple of 4 within [4, 1024])", C);
  GVK_REQUIRE(K >= 1 && K <= 65535, "gvk_scatter_matrix: K = %d classes outside [1, 65535]", K);
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)mean & 15) == 0 && ((uintptr_t)scratch & 7) == 0,
              "gvk_scatter_matrix: x and mean must be 16-byte aligned, scratch 8-byte aligned");
  int nt, npairs, nchunks, cps, nslabs;
  scat_split(N, C, nt, npairs, nchunks, cps, nslabs);
  const int64_t part_words = (int64_t)nslabs * npairs * kScatTile * kScatTile;
  const int64_t need = (part_words + nchunks) * (int64_t)sizeof(double);
  GVK_REQUIRE(scratch_bytes >= need, "gvk_scatter_matrix: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
  double* part = (double*)scratch;
  double* r4part = part + part_words;
  hipStream_t st = (hipStream_t)stream;
  GVK_LAUNCH(scatter_tile_kernel, dim3((unsigned)npairs, (unsigned)nslabs), dim3(256), 0, st, x, (const int*)labels, mean, part, N, C, K, nt, cps);
  GVK_LAUNCH(scatter_rows_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, x, (const int*)labels, mean, r4part, N, C, K);
  GVK_LAUNCH(scatter_finish_kernel, dim3((unsigned)(npairs * 16 + 1 + (K + 3) / 4)), dim3(256), 0, st, (const double*)part, (const double*)r4part,
             (const int*)labels, S, r4, (int*)count, N, C, K, nt, npairs, nslabs, nchunks);
  return check_launch("scatter_matrix");
}

extern "C" int gvk_mahalanobis(const float* q, const float* W, const float* m, float* d2, int Nq, int C, int K, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(q && W && m && d2, "gvk_mahalanobis: bad arguments");
  GVK_REQUIRE(Nq >= 1, "gvk_mahalanobis: Nq = %d (at least 1)", Nq);
  GVK_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, "gvk_mahalanobis: C = %d (a multiple of 4 within [4, 1024])", C);
  GVK_REQUIRE(K >= 1 && K <= kMahaMaxK, "gvk_mahalanobis: K = %d centres outside [1, %d]", K, kMahaMaxK);
  GVK_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)m & 15) == 0, "gvk_mahalanobis: q, W and m must be 16-byte aligned");
  const int KT = K <= 16 ? 1 : 2, KK = 16 * KT;
  const int Cp = ((C + 15) / 16) * 16;
  const size_t lds = (size_t)(16 * (Cp + 4) + kMahaWaves * KK * 17 + kMahaWaves * 16 * KK) * sizeof(float);
  const dim3 grid((unsigned)((Nq + 15) / 16)), block(64 * kMahaWaves);
  static size_t granted1 = 64 * 1024, granted2 = 64 * 1024;
  if (KT == 1) {
    if (int rc = ensure_lds(&mahalanobis_kernel<1>, lds, granted1, "mahalanobis<1>")) return rc;
    GVK_LAUNCH(mahalanobis_kernel<1>, grid, block, (unsigned)lds, (hipStream_t)stream, q, W, m, d2, Nq, C, K);
  } else {
    if (int rc = ensure_lds(&mahalanobis_kernel<2>, lds, granted2, "mahalanobis<2>")) return rc;
    GVK_LAUNCH(mahalanobis_kernel<2>, grid, block, (unsigned)lds, (hipStream_t)stream, q, W, m, d2, Nq, C, K);
  }
  return check_launch("mahalanobis");
}

extern "C" int gvk_logit_scores(const float* logits, float* out, int N, int K, float temperature, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(logits && out && N >= 1, "gvk_logit_scores: bad arguments");
  GVK_REQUIRE(K >= 2 && K <= 64 * kLogitKPL, "gvk_logit_scores: K = %d classes outside [2, %d]", K, 64 * kLogitKPL);
  GVK_REQUIRE(temperature > 0.f && temperature < INFINITY, "gvk_logit_scores: temperature = %g (a finite positive number)", (double)temperature);
  GVK_LAUNCH(logit_scores_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, out, N, K, (double)temperature);
  return check_launch("logit_scores");
}
