// Intensity normalisation on the device: tio.RescaleIntensity(out_min_max, percentiles, masking_method) and tio.ZNormalization(masking_method)
// on a batch of fp32 volumes x [B][V] resident in HBM, 1 <= V < 2^31, no divisibility requirement on V and no host read anywhere.
//
//   gvk_volume_stats        min / max / float64 mean of every voxel, then count, float64 mean and unbiased std of the masked voxels (x > t)
//   gvk_volume_order_stats  exact order statistics of the masked voxels by a most-significant-first radix select, 11 / 11 / 10 bits
//   gvk_normalize_intensity a tiny step that turns those tables into per-sample parameters and a status word, and one streaming apply pass
// and tio.HistogramStandardization on the same machinery:
//   gvk_volume_landmarks    the same order statistics at up to 16 percentiles in four sweeps of 8-bit digits, whatever the ranks fall under
//   gvk_histogram_standardize  per-sample piecewise-linear map from the volume's landmarks onto trained ones, and its streaming apply pass
//
// Every streaming kernel walks a sample the same way (stream_slab): sample b starts at x + b V, which is 16-byte aligned only when b V is a
// multiple of 4, so a sample is cut into a head of 0..3 voxels up to the next 16-byte boundary, a body of 16-byte loads shared out in equal
// contiguous slabs, and a tail of 0..3 voxels.  Sums are float64, per thread in ascending index order, then a fixed tree over the 256 threads
// and a fixed tree over the slabs: no floating-point atomics, the same bits on every run.  The only atomics are integer adds of the select's
// histograms, which are exact in any order.  NaN input is out of scope (a NaN fails every compare and is never counted).
#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

constexpr int kNmSlabs = GVK_NORMALIZE_SLABS;                    // slabs (workgroups) per sample, at most
constexpr int kNmBins = 2048;                                    // bins of one radix digit (11 bits; the last digit uses 1024 of them)
constexpr int kNmRanks = 2 * GVK_NORMALIZE_MAX_PERCENTILES;      // wanted ranks per sample: (a, b) of every percentile
constexpr int kNmSweep = 4;                                      // distinct prefixes one sweep over the data counts: 4 x 2048 bins = 32 KB LDS
constexpr int kSelWords = 32;                                    // per-sample select state, uint32: see order_init_kernel
constexpr int kStatWords = 8;                                    // per-sample statistics, double: GVK_NORMALIZE_STATS

// f(value, ok) for every voxel of slab `slab` of sample xb; every thread of the workgroup makes the same number of calls (ok = false where
// it has no voxel), so f may use wave-wide operations.  Four independent 16-byte loads are in flight per lane.
template <typename F>
__device__ __forceinline__ void stream_slab(const float* __restrict__ xb, long long V, int slab, int nslabs, F&& f) {
  const int tid = threadIdx.x;
  long long head = (long long)((4 - (int)(((uintptr_t)xb >> 2) & 3)) & 3);
  head = head < V ? head : V;
  const long long n4 = (V - head) >> 2;
  const f32x4* x4 = (const f32x4*)(xb + head);
  const long long per = (n4 + nslabs - 1) / nslabs;
  const long long i0 = (long long)slab * per, i1 = min(n4, i0 + per);
  for (long long base = i0; base < i1; base += 1024) {
    f32x4 v[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = base + 256 * u + tid;
      ok[u] = i < i1;
      v[u] = ok[u] ? x4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) f(v[u][e], ok[u]);
  }
  if (slab == 0) {                                               // head voxels on lanes 0..2 of wave 0, tail voxels on lanes 0..2 of wave 1
    const long long t0 = head + (n4 << 2);
    bool ok = false;
    float v = 0.f;
    if (tid < head) { v = xb[tid]; ok = true; }
    else if (tid >= 64 && t0 + (tid - 64) < V) { v = xb[t0 + (tid - 64)]; ok = true; }
    f(v, ok);
  }
}

// fixed-order tree over the 256 threads; the result is valid on thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = __dadd_rn(sh[tid], sh[tid + s]);
    __syncthreads();
  }
  return sh[0];
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// part [B][kNmSlabs][4] doubles.  STAGE 0: (min, max, sum) of every voxel.  STAGE 1: (count, sum) of the voxels above the threshold
// stats[3].  STAGE 2: sum of squared deviations of those voxels from their mean stats[5].
template <int STAGE>
__global__ __launch_bounds__(256) void volume_stats_kernel(const float* __restrict__ x, const double* __restrict__ stats, double* __restrict__ part,
                                                           long long V, int nslabs) {
  __shared__ double sh[256];
  __shared__ float smin[256], smax[256];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (size_t)b * V;
  double* out = part + ((size_t)b * kNmSlabs + slab) * 4;
  if (STAGE == 0) {
    float lo = INFINITY, hi = -INFINITY;
    double sum = 0.0;
    stream_slab(xb, V, slab, nslabs, [&](float v, bool ok) {
      if (ok) { lo = fminf(lo, v); hi = fmaxf(hi, v); sum = __dadd_rn(sum, (double)v); }
    });
    smin[tid] = lo; smax[tid] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) { smin[tid] = fminf(smin[tid], smin[tid + s]); smax[tid] = fmaxf(smax[tid], smax[tid + s]); }
      __syncthreads();
    }
    const double total = block_sum(sum, sh);
    if (tid == 0) { out[0] = (double)smin[0]; out[1] = (double)smax[0]; out[2] = total; }
  } else if (STAGE == 1) {
    const float t = (float)stats[(size_t)b * kStatWords + 3];
    double sum = 0.0;
    long long cnt = 0;
    stream_slab(xb, V, slab, nslabs, [&](float v, bool ok) {
      if (ok && v > t) { ++cnt; sum = __dadd_rn(sum, (double)v); }
    });
    const double n = block_sum((double)cnt, sh);                 // counts stay below 2^31: exact in float64
    const double total = block_sum(sum, sh);
    if (tid == 0) { out[0] = n; out[1] = total; }
  } else {
    const float t = (float)stats[(size_t)b * kStatWords + 3];
    const double mean = stats[(size_t)b * kStatWords + 5];
    double ss = 0.0;
    stream_slab(xb, V, slab, nslabs, [&](float v, bool ok) {
      if (ok && v > t) { const double d = __dsub_rn((double)v, mean); ss = __dadd_rn(ss, __dmul_rn(d, d)); }
    });
    const double total = block_sum(ss, sh);
    if (tid == 0) out[0] = total;
  }
}

// One 128-thread workgroup per sample folds the slabs in a fixed tree and writes the statistics table:
// stats [B][8] = (min, max, mean of all voxels, threshold, n, mean of the masked voxels, unbiased std of the masked voxels, unused).
__global__ __launch_bounds__(128) void volume_stats_finish_kernel(const double* __restrict__ part, double* __restrict__ stats, long long* __restrict__ count,
                                                                  long long V, int nslabs, int stage, int mask_mode, float threshold) {
  __shared__ double s0[128], s1[128], s2[128];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* p = part + ((size_t)b * kNmSlabs + tid) * 4;
  const bool have = tid < nslabs;
  if (stage == 0) { s0[tid] = have ? p[0] : (double)INFINITY; s1[tid] = have ? p[1] : -(double)INFINITY; s2[tid] = have ? p[2] : 0.0; }
  else { s0[tid] = have ? p[0] : 0.0; s1[tid] = (have && stage == 1) ? p[1] : 0.0; s2[tid] = 0.0; }
  __syncthreads();
  for (int s = 64; s > 0; s >>= 1) {
    if (tid < s) {
      if (stage == 0) { s0[tid] = fmin(s0[tid], s0[tid + s]); s1[tid] = fmax(s1[tid], s1[tid + s]); s2[tid] = __dadd_rn(s2[tid], s2[tid + s]); }
      else { s0[tid] = __dadd_rn(s0[tid], s0[tid + s]); s1[tid] = __dadd_rn(s1[tid], s1[tid + s]); }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  double* st = stats + (size_t)b * kStatWords;
  long long n = 0;
  if (stage == 0) {
    const double mean = __ddiv_rn(s2[0], (double)V);
    st[0] = s0[0]; st[1] = s1[0]; st[2] = mean;
    st[3] = mask_mode == 0 ? -(double)INFINITY : (mask_mode == 1 ? (double)(float)mean : (double)threshold);
    st[4] = (double)V; st[5] = mean; st[6] = 0.0; st[7] = 0.0;   // no mask: n and the masked mean are those of the whole volume
    n = V;
  } else if (stage == 1) {
    n = (long long)s0[0];
    st[4] = s0[0];
    st[5] = n > 0 ? __ddiv_rn(s1[0], s0[0]) : 0.0;
  } else {
    n = (long long)st[4];
    st[6] = n >= 2 ? __dsqrt_rn(__ddiv_rn(s0[0], (double)(n - 1))) : 0.0;
  }
  count[b] = n;
}

// ---- exact order statistics ------------------------------------------------------------------------------------------------------
// order-preserving key of a finite float: -0.0 is taken as +0.0 (they compare equal), negative values have every bit flipped,
// non-negative ones the sign bit.  Pure bit operations: denormals are ordinary keys.
__device__ __forceinline__ unsigned order_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// the virtual index of percentile fraction qf among n values, as numpy takes it: one float64 multiply
__device__ __forceinline__ void order_ranks(long long n, double qf, long long& ia, long long& ib, double& g) {
  const double v = __dmul_rn((double)(n - 1), qf);
  double i = floor(v);
  i = i < 0.0 ? 0.0 : (i > (double)(n - 1) ? (double)(n - 1) : i);
  ia = (long long)i;
  ib = ia + 1 < n ? ia + 1 : n - 1;
  g = __dsub_rn(v, i);
}

// Per-sample select state sel [B][32] uint32:
//   [0] nslots = distinct key prefixes the wanted ranks fall under (0: empty mask), [1..8] the prefixes (the key bits decided so far, right
//   aligned), [9..16] the slot of each of the 8 ranks, [17..24] each rank's position among the keys of its slot.
// One workgroup per sample writes the first state (every rank under the empty prefix) and zeroes the sample's histograms
// hist [B][3 passes][8 slots][2048] uint32.  Ranks beyond 2 Q repeat rank 0, so they never add a prefix.
__global__ __launch_bounds__(256) void order_init_kernel(const double* __restrict__ stats, unsigned* __restrict__ sel, unsigned* __restrict__ hist, int Q,
                                                         double q0, double q1, double q2, double q3) {
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned* h = hist + (size_t)b * 3 * kNmRanks * kNmBins;
  for (int i = tid; i < 3 * kNmRanks * kNmBins; i += 256) h[i] = 0u;
  if (tid != 0) return;
  unsigned* s = sel + (size_t)b * kSelWords;
  const long long n = (long long)stats[(size_t)b * kStatWords + 4];
  const double qf[4] = {q0, q1, q2, q3};
  for (int i = 0; i < kSelWords; ++i) s[i] = 0u;
  if (n <= 0) return;
  s[0] = 1u;
  for (int r = 0; r < kNmRanks; ++r) {
    const int q = r >> 1 < Q ? r >> 1 : 0;
    long long ia, ib;
    double g;
    order_ranks(n, qf[q], ia, ib, g);
    s[17 + r] = (unsigned)((r & 1) && (r >> 1) < Q ? ib : ia);
  }
}

// One add per distinct bin and wave where it matters: the bin most lanes hit last time (cand) and the first remaining lane's bin are each
// added once with their lane count, every other lane adds 1 for itself.  A volume whose background fills one bin would otherwise
// serialise 64 deep on that LDS word.  idx < 0: the lane has nothing to count.  Called by whole waves.
__device__ __forceinline__ void wave_count(unsigned* h, int idx, int& cand) {
  if (__ballot(idx >= 0) == 0ull) return;
  const int lane = lane_id();
  const unsigned long long m1 = __ballot(idx >= 0 && idx == cand);
  if (m1 != 0ull && lane == __ffsll((long long)m1) - 1) atomicAdd(&h[idx], (unsigned)__popcll(m1));
  const bool mine = idx >= 0 && idx != cand;
  const unsigned long long rest = __ballot(mine);
  if (rest == 0ull) return;
  const int first = __ffsll((long long)rest) - 1;
  const int c2 = __shfl(idx, first, 64);
  const unsigned long long m2 = __ballot(mine && idx == c2);
  if (mine) {
    if (idx != c2) atomicAdd(&h[idx], 1u);
    else if (lane == first) atomicAdd(&h[idx], (unsigned)__popcll(m2));
  }
  if (__popcll(m2) > __popcll(m1)) cand = c2;
}

// Pass `pass` of the select: every workgroup counts, for its slab, the current digit of the masked keys whose higher bits equal one of
// the sample's wanted prefixes -- into an LDS histogram of up to 4 prefixes x 2048 bins, merged into the sample's global histogram with
// integer atomics (non-zero bins only).  More than 4 distinct prefixes (at most 8: one per rank) take a second sweep over the slab.
__global__ __launch_bounds__(256) void order_hist_kernel(const float* __restrict__ x, const double* __restrict__ stats, const unsigned* __restrict__ sel,
                                                         unsigned* __restrict__ hist, long long V, int nslabs, int pass) {
  __shared__ unsigned h[kNmSweep * kNmBins];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const unsigned* s = sel + (size_t)b * kSelWords;
  const int nslots = min((int)s[0], kNmRanks);
  const float t = (float)stats[(size_t)b * kStatWords + 3];
  const float* xb = x + (size_t)b * V;
  unsigned* gh = hist + ((size_t)b * 3 + pass) * kNmRanks * kNmBins;
  const int dshift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
  const unsigned dmask = pass == 2 ? 1023u : 2047u;
  const int pshift = pass == 1 ? 21 : 10;                         // pass 0 has the empty prefix
  for (int base = 0; base < nslots; base += kNmSweep) {
    const int ns = min(kNmSweep, nslots - base);
    unsigned pre[kNmSweep];
#pragma unroll
    for (int j = 0; j < kNmSweep; ++j) pre[j] = j < ns ? s[1 + base + j] : 0u;
    for (int i = tid; i < ns * kNmBins; i += 256) h[i] = 0u;
    __syncthreads();
    int cand = -2;
    stream_slab(xb, V, slab, nslabs, [&](float v, bool ok) {
      int idx = -1;
      if (ok && v > t) {
        const unsigned key = order_key(v);
        const unsigned hp = pass == 0 ? 0u : key >> pshift;
        const int d = (int)((key >> dshift) & dmask);
#pragma unroll
        for (int j = 0; j < kNmSweep; ++j)
          if (j < ns && hp == pre[j]) idx = j * kNmBins + d;
      }
      wave_count(h, idx, cand);
    });
    __syncthreads();
    for (int i = tid; i < ns * kNmBins; i += 256) {
      const unsigned c = h[i];
      if (c != 0u) atomicAdd(&gh[base * kNmBins + i], c);
    }
    __syncthreads();
  }
}

// Between passes, one workgroup per sample: for every rank, the bin of its slot's histogram that holds it and its position inside that bin;
// then the new list of distinct prefixes.  After the last pass the prefixes are whole keys: write the pairs (a, b) and the cutoffs
// c = a + (b - a) g for g < 0.5, b - (b - a) (1 - g) otherwise, in float64 with one rounding per operation, rounded to float32 at the end.
__global__ __launch_bounds__(256) void order_select_kernel(const double* __restrict__ stats, unsigned* sel, const unsigned* __restrict__ hist,
                                                           float* __restrict__ pairs, float* __restrict__ cutoffs, int Q, double q0, double q1,
                                                           double q2, double q3, int pass) {
  __shared__ unsigned sc[256];
  __shared__ unsigned rbin[kNmRanks], rpos[kNmRanks];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned* s = sel + (size_t)b * kSelWords;
  const int nslots = min((int)s[0], kNmRanks);
  const int bits = pass == 2 ? 10 : 11;
  if (tid < kNmRanks) { rbin[tid] = 0u; rpos[tid] = 0u; }
  __syncthreads();
  for (int slot = 0; slot < nslots; ++slot) {
    const unsigned* gh = hist + (((size_t)b * 3 + pass) * kNmRanks + slot) * kNmBins + tid * 8;
    unsigned c[8], tot = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = gh[j]; tot += c[j]; }
    sc[tid] = tot;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                    // inclusive scan of the 256 thread totals
      const unsigned add = tid >= off ? sc[tid - off] : 0u;
      __syncthreads();
      sc[tid] += add;
      __syncthreads();
    }
    const unsigned excl = sc[tid] - tot;
    for (int r = 0; r < kNmRanks; ++r) {
      const unsigned rk = s[17 + r];
      if ((int)s[9 + r] == slot && rk >= excl && rk - excl < tot) {
        unsigned before = excl;
        for (int j = 0; j < 8; ++j) {
          if (rk - before < c[j]) { rbin[r] = (unsigned)(tid * 8 + j); rpos[r] = rk - before; break; }
          before += c[j];
        }
      }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  unsigned key[kNmRanks], npre[kNmRanks], nslot[kNmRanks];
  int ns = 0;
  if (nslots > 0)
    for (int r = 0; r < kNmRanks; ++r) {
      const int old = min((int)s[9 + r], kNmRanks - 1);
      key[r] = (s[1 + old] << bits) | rbin[r];
      int j = 0;
      while (j < ns && npre[j] != key[r]) ++j;
      if (j == ns) npre[ns++] = key[r];
      nslot[r] = (unsigned)j;
    }
  if (nslots > 0) {
    s[0] = (unsigned)ns;
    for (int j = 0; j < kNmRanks; ++j) s[1 + j] = j < ns ? npre[j] : 0u;
    for (int r = 0; r < kNmRanks; ++r) { s[9 + r] = nslot[r]; s[17 + r] = rpos[r]; }
  }
  if (pass != 2) return;
  const long long n = (long long)stats[(size_t)b * kStatWords + 4];
  const double qf[4] = {q0, q1, q2, q3};
  for (int q = 0; q < Q; ++q) {
    float fa = 0.f, fb = 0.f, fc = 0.f;                          // empty mask: zeros, and status 1 from gvk_normalize_intensity
    if (nslots > 0 && n > 0) {
      fa = order_value(key[2 * q]);
      fb = order_value(key[2 * q + 1]);
      long long ia, ib;
      double g;
      order_ranks(n, qf[q], ia, ib, g);
      const double a = (double)fa, bb = (double)fb, diff = __dsub_rn(bb, a);
      const double c = g < 0.5 ? __dadd_rn(a, __dmul_rn(diff, g)) : __dsub_rn(bb, __dmul_rn(diff, __dsub_rn(1.0, g)));
      fc = (float)c;
    }
    pairs[((size_t)b * Q + q) * 2] = fa;
    pairs[((size_t)b * Q + q) * 2 + 1] = fb;
    cutoffs[(size_t)b * Q + q] = fc;
  }
}

// ---- parameters and apply --------------------------------------------------------------------------------------------------------
// params [B][8] doubles = (lo, hi, sub, div, mul, add, mean, std); the float32 quantities of the rescale are stored exactly.
// status [B]: 0 normalised, 1 empty mask, 2 in_range == 0 / std == 0 / n < 2 -- a sample with a non-zero status is copied bit for bit.
__global__ void normalize_params_kernel(const double* __restrict__ stats, const float* __restrict__ cutoffs, int Q, double* __restrict__ params,
                                        int* __restrict__ status, int mode, float out_min, float out_max, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* st = stats + (size_t)b * kStatWords;
  double* p = params + (size_t)b * 8;
  const long long n = (long long)st[4];
  int code = 0;
  for (int i = 0; i < 8; ++i) p[i] = 0.0;
  if (mode == GVK_NORMALIZE_RESCALE) {
    const float lo = cutoffs[(size_t)b * Q], hi = cutoffs[(size_t)b * Q + 1];
    const float mn = (float)st[0], mx = (float)st[1];
    const float in_min = fminf(fmaxf(mn, lo), hi), in_max = fminf(fmaxf(mx, lo), hi);   // min and max of the clipped volume
    const float in_range = in_max - in_min;
    p[0] = lo; p[1] = hi; p[2] = in_min; p[3] = in_range; p[4] = out_max - out_min; p[5] = out_min;
    code = n <= 0 ? 1 : (in_range == 0.f ? 2 : 0);
  } else {
    p[6] = st[5]; p[7] = st[6];
    code = n <= 0 ? 1 : ((n < 2 || st[6] == 0.0) ? 2 : 0);
  }
  status[b] = code;
}

__device__ __forceinline__ float normalize_one(float v, int mode, float lo, float hi, float sub, float div, float mul, float add, double mean, double sd) {
  if (mode == GVK_NORMALIZE_RESCALE) {
    float t = v > lo ? v : lo;                                    // numpy's clip: max, then min
    t = t < hi ? t : hi;
    t = t - sub;
    t = t / div;                                                  // a true divide, as torchio's x /= in_range
    t = t * mul;
    return t + add;
  }
  return (float)__ddiv_rn(__dsub_rn((double)v, mean), sd);
}

__global__ __launch_bounds__(256) void normalize_apply_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ params,
                                                              const int* __restrict__ status, long long V, int mode) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* p = params + (size_t)b * 8;
  const int m = status[b] != 0 ? -1 : mode;                       // -1: copy
  const float lo = (float)p[0], hi = (float)p[1], sub = (float)p[2], div = (float)p[3], mul = (float)p[4], add = (float)p[5];
  const double mean = p[6], sd = p[7];
  const float* xb = x + (size_t)b * V;
  float* yb = y + (size_t)b * V;
  long long head = (long long)((4 - (int)(((uintptr_t)xb >> 2) & 3)) & 3);   // x and y are 16-byte aligned: yb has the same head
  head = head < V ? head : V;
  const long long n4 = (V - head) >> 2;
  const f32x4* x4 = (const f32x4*)(xb + head);
  f32x4* y4 = (f32x4*)(yb + head);
  for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = x4[i];
    if (m >= 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = normalize_one(v[e], m, lo, hi, sub, div, mul, add, mean, sd);
    }
    y4[i] = v;
  }
  if (blockIdx.x == 0) {
    const long long t0 = head + (n4 << 2);
    long long i = -1;
    if (tid < head) i = tid;
    else if (tid >= 64 && t0 + (tid - 64) < V) i = t0 + (tid - 64);
    if (i >= 0) {
      const float v = xb[i];
      yb[i] = m >= 0 ? normalize_one(v, m, lo, hi, sub, div, mul, add, mean, sd) : v;
    }
  }
}

static int normalize_slabs(int64_t V) { return (int)std::min<int64_t>(kNmSlabs, std::max<int64_t>(1, (V / 4 + 1023) / 1024)); }

// ---- landmarks: up to 16 order statistics in a fixed number of sweeps ----------------------------------------------------------------
// tio.HistogramStandardization needs 13 percentiles of every volume to train and 11 to apply.  The select above counts 4 prefixes per sweep;
// this one gives every one of the 2 Q <= 32 wanted ranks a slot of its own, so a pass is ONE sweep whatever the ranks fall under: four passes
// of 8-bit digits, 32 slots x 256 bins = 32 KB of LDS.  Ranks, keys, the contention trick and the cutoff arithmetic are those of the select
// above, so the results are its results bit for bit.
constexpr int kLmRanks = 2 * GVK_LANDMARKS_MAX;                  // rank slots: (a, b) of every percentile
constexpr int kLmBins = 256;                                     // bins of one 8-bit digit
constexpr int kLmPasses = 4;
constexpr int kLmSelWords = 128;                                 // per-sample select state, uint32: see landmark_init_kernel
constexpr int kHsKnots = GVK_HISTSTD_KNOTS;                      // 11 knots, 10 segments
constexpr int kHsParams = GVK_HISTSTD_PARAMS;                    // per-sample doubles: knots [0..10], slopes [11..20], intercepts [21..30]
static_assert(kLmSelWords + kLmPasses * kLmRanks * kLmBins == GVK_LANDMARKS_WS_WORDS, "workspace size");

struct LandmarkFractions { double q[GVK_LANDMARKS_MAX]; };       // a kernel argument: the fractions never touch device memory
struct HistogramTargets { double m[kHsKnots]; };

// Per-sample select state sel [B][128] uint32:
//   [0] nslots = distinct key prefixes the wanted ranks fall under (0: empty mask), [1..32] the prefixes (the key bits decided so far, right
//   aligned), [33..64] the slot of each of the 32 ranks, [65..96] each rank's position among the keys of its slot.
// One workgroup per sample writes the first state and zeroes the sample's histograms hist [B][4 passes][32 slots][256].  Ranks beyond 2 Q
// repeat rank 0, so they never add a prefix.
__global__ __launch_bounds__(256) void landmark_init_kernel(const double* __restrict__ stats, unsigned* __restrict__ sel, unsigned* __restrict__ hist, int Q,
                                                            LandmarkFractions f) {
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned* h = hist + (size_t)b * kLmPasses * kLmRanks * kLmBins;
  for (int i = tid; i < kLmPasses * kLmRanks * kLmBins; i += 256) h[i] = 0u;
  if (tid >= kLmSelWords) return;
  unsigned* s = sel + (size_t)b * kLmSelWords;
  const long long n = (long long)stats[(size_t)b * kStatWords + 4];
  unsigned word = 0u;
  if (n > 0) {
    if (tid == 0) word = 1u;
    if (tid >= 65 && tid < 65 + kLmRanks) {
      const int r = tid - 65;
      const bool mine = (r >> 1) < Q;
      double qf = f.q[0];
#pragma unroll
      for (int j = 1; j < GVK_LANDMARKS_MAX; ++j) qf = (mine && (r >> 1) == j) ? f.q[j] : qf;
      long long ia, ib;
      double g;
      order_ranks(n, qf, ia, ib, g);
      word = (unsigned)((r & 1) && mine ? ib : ia);
    }
  }
  s[tid] = word;
}

// NS = the slots this instantiation compares against (unused ones hold a prefix no key has)
template <int NS>
__device__ __forceinline__ void landmark_sweep(unsigned* h, const unsigned* __restrict__ s, int ns, const float* __restrict__ xb, long long V, int slab,
                                               int nslabs, float t, int pass) {
  unsigned pre[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) pre[j] = j < ns ? s[1 + j] : 0xffffffffu;   // prefixes have at most 24 bits
  const int dshift = 24 - 8 * pass;
  int cand = -2;
  stream_slab(xb, V, slab, nslabs, [&](float v, bool ok) {
    int idx = -1;
    if (ok && v > t) {
      const unsigned key = order_key(v);
      const unsigned hp = pass == 0 ? 0u : key >> (dshift + 8);
      const int d = (int)((key >> dshift) & 255u);
#pragma unroll
      for (int j = 0; j < NS; ++j)
        if (hp == pre[j]) idx = j * kLmBins + d;
    }
    wave_count(h, idx, cand);
  });
}

// Pass `pass`: every workgroup counts, for its slab, the current digit of the masked keys whose higher bits equal one of the sample's
// prefixes, in ONE sweep, and merges its non-zero bins into the sample's histogram with integer atomics.
__global__ __launch_bounds__(256) void landmark_hist_kernel(const float* __restrict__ x, const double* __restrict__ stats, const unsigned* __restrict__ sel,
                                                            unsigned* __restrict__ hist, long long V, int nslabs, int pass) {
  __shared__ unsigned h[kLmRanks * kLmBins];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const unsigned* s = sel + (size_t)b * kLmSelWords;
  const int ns = min((int)s[0], kLmRanks);
  if (ns == 0) return;                                           // empty mask: nothing to count (uniform over the workgroup)
  const float t = (float)stats[(size_t)b * kStatWords + 3];
  const float* xb = x + (size_t)b * V;
  unsigned* gh = hist + ((size_t)b * kLmPasses + pass) * kLmRanks * kLmBins;
  for (int i = tid; i < ns * kLmBins; i += 256) h[i] = 0u;
  __syncthreads();
  if (ns <= 1) landmark_sweep<1>(h, s, ns, xb, V, slab, nslabs, t, pass);
  else if (ns <= 8) landmark_sweep<8>(h, s, ns, xb, V, slab, nslabs, t, pass);
  else if (ns <= 16) landmark_sweep<16>(h, s, ns, xb, V, slab, nslabs, t, pass);
  else landmark_sweep<kLmRanks>(h, s, ns, xb, V, slab, nslabs, t, pass);
  __syncthreads();
  for (int i = tid; i < ns * kLmBins; i += 256) {
    const unsigned c = h[i];
    if (c != 0u) atomicAdd(&gh[i], c);
  }
}

// Between passes, one workgroup per sample.  Each wave takes every fourth slot: a lane holds 4 bins, a shuffle scan gives their offsets, and
// the lane whose bins hold a rank of that slot notes the bin and the rank's position in it.  Then lanes 0..31 build the new state: rank r's
// new prefix, the first rank with the same prefix, and from the ballot of those firsts the compacted slot numbers.  After the last pass the
// prefixes are whole keys: pairs and cutoffs as in order_select_kernel.
__global__ __launch_bounds__(256) void landmark_select_kernel(const double* __restrict__ stats, unsigned* sel, const unsigned* __restrict__ hist,
                                                              float* __restrict__ pairs, float* __restrict__ cutoffs, int Q, LandmarkFractions f, int pass) {
  __shared__ unsigned rbin[kLmRanks], rpos[kLmRanks], skey[kLmRanks];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* s = sel + (size_t)b * kLmSelWords;
  const int nslots = min((int)s[0], kLmRanks);
  if (tid < kLmRanks) { rbin[tid] = 0u; rpos[tid] = 0u; skey[tid] = 0u; }
  __syncthreads();
  for (int slot = wave; slot < nslots; slot += 4) {
    const unsigned* gh = hist + (((size_t)b * kLmPasses + pass) * kLmRanks + slot) * kLmBins + lane * 4;
    unsigned c[4], tot = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = gh[j]; tot += c[j]; }
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned up = __shfl_up(inc, off, 64);
      if (lane >= off) inc += up;
    }
    const unsigned excl = inc - tot;
    for (int r = 0; r < kLmRanks; ++r) {
      const unsigned rk = s[65 + r];
      if ((int)s[33 + r] == slot && rk >= excl && rk - excl < tot) {
        unsigned before = excl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (rk - before < c[j]) { rbin[r] = (unsigned)(lane * 4 + j); rpos[r] = rk - before; break; }
          before += c[j];
        }
      }
    }
  }
  __syncthreads();
  const bool act = tid < kLmRanks && nslots > 0;
  unsigned key = 0u;
  if (act) {
    const int old = min((int)s[33 + tid], kLmRanks - 1);
    key = (s[1 + old] << 8) | rbin[tid];
    skey[tid] = key;
  }
  __syncthreads();                                               // every read of the old state lies before this barrier
  if (tid >= 64) return;
  int first = tid;
  if (act)
    for (int j = tid - 1; j >= 0; --j)
      if (skey[j] == key) first = j;
  const unsigned long long firsts = __ballot(act && first == tid);
  if (act) {
    const int slot = __popcll(firsts & ((1ull << first) - 1ull));
    s[33 + tid] = (unsigned)slot;
    s[65 + tid] = rpos[tid];
    if (first == tid) s[1 + slot] = key;
    if (tid == 0) s[0] = (unsigned)__popcll(firsts);
  }
  if (pass != kLmPasses - 1 || tid >= Q) return;
  const long long n = (long long)stats[(size_t)b * kStatWords + 4];
  float fa = 0.f, fb = 0.f, fc = 0.f;                            // empty mask: zeros, and status 1 from gvk_histogram_standardize
  if (nslots > 0 && n > 0) {
    fa = order_value(skey[2 * tid]);
    fb = order_value(skey[2 * tid + 1]);
    double qf = f.q[0];
#pragma unroll
    for (int j = 1; j < GVK_LANDMARKS_MAX; ++j) qf = tid == j ? f.q[j] : qf;
    long long ia, ib;
    double g;
    order_ranks(n, qf, ia, ib, g);
    const double a = (double)fa, bb = (double)fb, diff = __dsub_rn(bb, a);
    const double c = g < 0.5 ? __dadd_rn(a, __dmul_rn(diff, g)) : __dsub_rn(bb, __dmul_rn(diff, __dsub_rn(1.0, g)));
    fc = (float)c;
  }
  pairs[((size_t)b * Q + tid) * 2] = fa;
  pairs[((size_t)b * Q + tid) * 2 + 1] = fb;
  cutoffs[(size_t)b * Q + tid] = fc;
}

// ---- histogram standardisation: parameters and apply -----------------------------------------------------------------------------------
// torchio's _normalize on float64: d_j = k_{j+1} - k_j, taken as inf below epsilon (slope 0); slope_j = (m_{j+1} - m_j) / d_j;
// icpt_j = m_j - slope_j k_j.  params [B][32] doubles = knots [0..10] (the float32 cutoffs), slopes [11..20], intercepts [21..30].
// status [B]: 0 standardised, 1 empty mask -- such a sample is copied bit for bit.
__global__ void histstd_params_kernel(const double* __restrict__ stats, const float* __restrict__ cutoffs, HistogramTargets tg, double epsilon,
                                      double* __restrict__ params, int* __restrict__ status, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* p = params + (size_t)b * kHsParams;
  const float* c = cutoffs + (size_t)b * kHsKnots;
  for (int i = 0; i < kHsParams; ++i) p[i] = 0.0;
  for (int j = 0; j < kHsKnots; ++j) p[j] = (double)c[j];
  for (int j = 0; j + 1 < kHsKnots; ++j) {
    const double k0 = (double)c[j];
    double d = __dsub_rn((double)c[j + 1], k0);
    if (d < epsilon) d = (double)INFINITY;
    const double slope = __ddiv_rn(__dsub_rn(tg.m[j + 1], tg.m[j]), d);
    p[kHsKnots + j] = slope;
    p[2 * kHsKnots - 1 + j] = __dsub_rn(tg.m[j], __dmul_rn(slope, k0));
  }
  status[b] = (long long)stats[(size_t)b * kStatWords + 4] <= 0 ? 1 : 0;
}

// The segment of x is the number of interior knots k_1..k_9 that are <= x (np.digitize, right=False); the knots ascend, so the last
// knot that is <= x names it: nine float32 compares, each selecting that segment's (slope, intercept).  y = float32(slope (double)x + icpt),
// the product and the sum rounded once each.
__device__ __forceinline__ float histstd_one(float v, const float (&k)[kHsKnots - 2], const double (&sl)[kHsKnots - 1], const double (&ic)[kHsKnots - 1]) {
  double s = sl[0], c = ic[0];
#pragma unroll
  for (int j = 0; j < kHsKnots - 2; ++j) {
    const bool at = v >= k[j];
    s = at ? sl[j + 1] : s;
    c = at ? ic[j + 1] : c;
  }
  return (float)__dadd_rn(__dmul_rn(s, (double)v), c);
}

// head / body / tail as normalize_apply_kernel: a sample may start off the 16-byte grid
__global__ __launch_bounds__(256) void histstd_apply_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ params,
                                                            const int* __restrict__ status, long long V) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* p = params + (size_t)b * kHsParams;
  const bool live = status[b] == 0;
  float k[kHsKnots - 2];
  double sl[kHsKnots - 1], ic[kHsKnots - 1];
#pragma unroll
  for (int j = 0; j < kHsKnots - 2; ++j) k[j] = (float)p[1 + j];
#pragma unroll
  for (int j = 0; j < kHsKnots - 1; ++j) { sl[j] = p[kHsKnots + j]; ic[j] = p[2 * kHsKnots - 1 + j]; }
  const float* xb = x + (size_t)b * V;
  float* yb = y + (size_t)b * V;
  long long head = (long long)((4 - (int)(((uintptr_t)xb >> 2) & 3)) & 3);   // x and y are 16-byte aligned: yb has the same head
  head = head < V ? head : V;
  const long long n4 = (V - head) >> 2;
  const f32x4* x4 = (const f32x4*)(xb + head);
  f32x4* y4 = (f32x4*)(yb + head);
  for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = x4[i];
    if (live) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = histstd_one(v[e], k, sl, ic);
    }
    y4[i] = v;
  }
  if (blockIdx.x == 0) {
    const long long t0 = head + (n4 << 2);
    long long i = -1;
    if (tid < head) i = tid;
    else if (tid >= 64 && t0 + (tid - 64) < V) i = t0 + (tid - 64);
    if (i >= 0) {
      const float v = xb[i];
      yb[i] = live ? histstd_one(v, k, sl, ic) : v;
    }
  }
}

}  // namespace gvk

extern "C" int gvk_volume_stats(const float* x, double* partials, double* stats, int64_t* count, int mask_mode, float threshold, int want_std, int B,
                                int64_t V, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && partials && stats && count, "gvk_volume_stats: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && V > 0 && V < ((int64_t)1 << 31), "gvk_volume_stats: 1 <= B <= 65535 and 1 <= V < 2^31");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0, "gvk_volume_stats: x must be 16-byte aligned");
  GVK_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "gvk_volume_stats: mask_mode is 0 (none), 1 (above the mean) or 2 (above threshold)");
  const int S = normalize_slabs(V);
  hipStream_t st = (hipStream_t)stream;
  const bool masked = mask_mode != 0;
  GVK_LAUNCH(volume_stats_kernel<0>, dim3(S, B), dim3(256), 0, st, x, (const double*)stats, partials, (long long)V, S);
  GVK_LAUNCH(volume_stats_finish_kernel, dim3(B), dim3(128), 0, st, (const double*)partials, stats, (long long*)count, (long long)V, S, 0, mask_mode,
             threshold);
  if (masked) {
    GVK_LAUNCH(volume_stats_kernel<1>, dim3(S, B), dim3(256), 0, st, x, (const double*)stats, partials, (long long)V, S);
    GVK_LAUNCH(volume_stats_finish_kernel, dim3(B), dim3(128), 0, st, (const double*)partials, stats, (long long*)count, (long long)V, S, 1, mask_mode,
               threshold);
  }
  if (want_std) {
    GVK_LAUNCH(volume_stats_kernel<2>, dim3(S, B), dim3(256), 0, st, x, (const double*)stats, partials, (long long)V, S);
    GVK_LAUNCH(volume_stats_finish_kernel, dim3(B), dim3(128), 0, st, (const double*)partials, stats, (long long*)count, (long long)V, S, 2, mask_mode,
               threshold);
  }
  return check_launch("volume_stats");
}

extern "C" int gvk_volume_order_stats(const float* x, const double* stats, void* workspace, float* pairs, float* cutoffs, int Q, double q0, double q1,
                                      double q2, double q3, int B, int64_t V, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && stats && workspace && pairs && cutoffs, "gvk_volume_order_stats: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && V > 0 && V < ((int64_t)1 << 31), "gvk_volume_order_stats: 1 <= B <= 65535 and 1 <= V < 2^31");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 3) == 0, "gvk_volume_order_stats: x must be 16-byte aligned");
  GVK_REQUIRE(Q >= 1 && Q <= GVK_NORMALIZE_MAX_PERCENTILES, "gvk_volume_order_stats: 1..%d percentiles per call", (int)GVK_NORMALIZE_MAX_PERCENTILES);
  const double qf[4] = {q0, q1, q2, q3};
  for (int q = 0; q < Q; ++q) GVK_REQUIRE(qf[q] >= 0.0 && qf[q] <= 1.0, "gvk_volume_order_stats: percentile fractions lie in [0, 1]");
  const int S = normalize_slabs(V);
  hipStream_t st = (hipStream_t)stream;
  unsigned* sel = (unsigned*)workspace;
  unsigned* hist = sel + (size_t)B * kSelWords;
  GVK_LAUNCH(order_init_kernel, dim3(B), dim3(256), 0, st, stats, sel, hist, Q, q0, q1, q2, q3);
  for (int pass = 0; pass < 3; ++pass) {
    GVK_LAUNCH(order_hist_kernel, dim3(S, B), dim3(256), 0, st, x, stats, (const unsigned*)sel, hist, (long long)V, S, pass);
    GVK_LAUNCH(order_select_kernel, dim3(B), dim3(256), 0, st, stats, sel, (const unsigned*)hist, pairs, cutoffs, Q, q0, q1, q2, q3, pass);
  }
  return check_launch("volume_order_stats");
}

extern "C" int gvk_normalize_intensity(const float* x, float* y, const double* stats, const float* cutoffs, int Q, double* params, int32_t* status,
                                       int mode, float out_min, float out_max, int B, int64_t V, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && y && stats && params && status, "gvk_normalize_intensity: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && V > 0 && V < ((int64_t)1 << 31), "gvk_normalize_intensity: 1 <= B <= 65535 and 1 <= V < 2^31");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "gvk_normalize_intensity: x and y must be 16-byte aligned");
  GVK_REQUIRE(mode == GVK_NORMALIZE_RESCALE || mode == GVK_NORMALIZE_ZNORM, "gvk_normalize_intensity: mode is GVK_NORMALIZE_RESCALE or GVK_NORMALIZE_ZNORM");
  GVK_REQUIRE(mode != GVK_NORMALIZE_RESCALE || (cutoffs && Q >= 2 && Q <= GVK_NORMALIZE_MAX_PERCENTILES),
              "gvk_normalize_intensity: the rescale reads cutoffs [B][Q], Q >= 2 (low, high first)");
  hipStream_t st = (hipStream_t)stream;
  GVK_LAUNCH(normalize_params_kernel, dim3((B + 63) / 64), dim3(64), 0, st, stats, cutoffs, Q, params, (int*)status, mode, out_min, out_max, B);
  const int gx = (int)std::min<int64_t>((V / 4 + 255) / 256 + 1, 512);
  GVK_LAUNCH(normalize_apply_kernel, dim3(gx, B), dim3(256), 0, st, x, y, (const double*)params, (const int*)status, (long long)V, mode);
  return check_launch("normalize_intensity");
}

extern "C" int gvk_volume_landmarks(const float* x, const double* stats, void* workspace, float* pairs, float* cutoffs, int Q, const double* fractions_host,
                                    int B, int64_t V, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && stats && workspace && pairs && cutoffs && fractions_host, "gvk_volume_landmarks: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && V > 0 && V < ((int64_t)1 << 31), "gvk_volume_landmarks: 1 <= B <= 65535 and 1 <= V < 2^31");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 3) == 0, "gvk_volume_landmarks: x must be 16-byte aligned");
  GVK_REQUIRE(Q >= 1 && Q <= GVK_LANDMARKS_MAX, "gvk_volume_landmarks: 1..%d percentiles per call", (int)GVK_LANDMARKS_MAX);
  LandmarkFractions f;
  for (int q = 0; q < GVK_LANDMARKS_MAX; ++q) f.q[q] = q < Q ? fractions_host[q] : 0.0;
  for (int q = 0; q < Q; ++q) GVK_REQUIRE(f.q[q] >= 0.0 && f.q[q] <= 1.0, "gvk_volume_landmarks: percentile fractions lie in [0, 1]");
  const int S = normalize_slabs(V);
  hipStream_t st = (hipStream_t)stream;
  unsigned* sel = (unsigned*)workspace;
  unsigned* hist = sel + (size_t)B * kLmSelWords;
  GVK_LAUNCH(landmark_init_kernel, dim3(B), dim3(256), 0, st, stats, sel, hist, Q, f);
  for (int pass = 0; pass < kLmPasses; ++pass) {
    GVK_LAUNCH(landmark_hist_kernel, dim3(S, B), dim3(256), 0, st, x, stats, (const unsigned*)sel, hist, (long long)V, S, pass);
    GVK_LAUNCH(landmark_select_kernel, dim3(B), dim3(256), 0, st, stats, sel, (const unsigned*)hist, pairs, cutoffs, Q, f, pass);
  }
  return check_launch("volume_landmarks");
}

extern "C" int gvk_histogram_standardize(const float* x, float* y, const double* stats, const float* cutoffs, const double* targets_host, double epsilon,
                                         double* params, int32_t* status, int B, int64_t V, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(x && y && stats && cutoffs && targets_host && params && status, "gvk_histogram_standardize: null pointer");
  GVK_REQUIRE(B > 0 && B <= 65535 && V > 0 && V < ((int64_t)1 << 31), "gvk_histogram_standardize: 1 <= B <= 65535 and 1 <= V < 2^31");
  GVK_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "gvk_histogram_standardize: x and y must be 16-byte aligned");
  GVK_REQUIRE(epsilon >= 0.0, "gvk_histogram_standardize: epsilon is not negative");
  HistogramTargets tg;
  for (int j = 0; j < kHsKnots; ++j) {
    tg.m[j] = targets_host[j];
    GVK_REQUIRE(std::isfinite(tg.m[j]), "gvk_histogram_standardize: the targets are finite");
  }
  hipStream_t st = (hipStream_t)stream;
  GVK_LAUNCH(histstd_params_kernel, dim3((B + 63) / 64), dim3(64), 0, st, stats, cutoffs, tg, epsilon, params, (int*)status, B);
  const int gx = (int)std::min<int64_t>((V / 4 + 255) / 256 + 1, 512);
  GVK_LAUNCH(histstd_apply_kernel, dim3(gx, B), dim3(256), 0, st, x, y, (const double*)params, (const int*)status, (long long)V);
  return check_launch("histogram_standardize");
}
