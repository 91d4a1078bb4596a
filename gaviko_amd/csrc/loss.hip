// Loss seed of the training step, forward and backward in ONE launch: train.py:176-179 (FocalLoss(gamma=1.2) or
// CrossEntropyLoss), 283/306 (loss = criterion(outputs, labels)) and the two per-step host reads of train.py:327-328
// (running loss, number of correct argmax predictions), which become device-side accumulators.
//
// FocalLoss is reproduced as it EXECUTES (losses/focal_loss.py:84-115): the live _process_preds clamps to [eps, 1-eps] and
// then softmaxes, and forward calls it twice, so
//   p1 = softmax(clamp(x)),  p2 = softmax(clamp(p1)),  pt = p2[target],  l = w_t (1-pt)^gamma * -log(eps + pt)
//   loss = sum l / sum (not ignored) w_t
// and the gradient flows back through both softmaxes and both clamps (zero for every logit outside [eps, 1-eps]).
// A label that is neither ignore_index nor a class (outside [0, K), compared as the 64-bit value it is) makes its row a BAD row: nothing is
// read at that index, the row's loss and its whole dlogits row are NaN, the reduced loss is NaN and the meter's correct count gains nothing.
// The step makes no host read, so the kernel cannot raise as torch does; NaN is the loud device-side equivalent.
// The logits are [B, K] with K a handful of classes: one workgroup, one thread per sample, every vector recomputed per pass
// instead of kept (no arrays, no scratch).
#include "common.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

struct LossArgs {
  const float* logits; const long long* target; const float* weights;
  float* loss; float* dlogits; float* meter;
  int B, K, kind, reduction;
  float gamma, eps, hi;
  long long ignore_index;
};

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

struct Soft1 { float m, s; };
// softmax statistics of clamp(x)
__device__ __forceinline__ Soft1 soft1(const float* x, int K, float lo, float hi) {
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, clampf(x[k], lo, hi));
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(clampf(x[k], lo, hi) - m);
  return {m, s};
}
__device__ __forceinline__ float p1_of(const float* x, int k, Soft1 a, float lo, float hi) { return expf(clampf(x[k], lo, hi) - a.m) / a.s; }

// ---- row arithmetic shared by loss_kernel and loss_mixed_kernel: every expression below is the one loss_kernel had inline, operation for
// operation (the library builds with -ffp-contract=off, so the order of the operations is the bits) ---------------------------------------
__device__ __forceinline__ int argmax_row(const float* x, int K) {  // torch.argmax: first maximum
  int am = 0;
  for (int k = 1; k < K; ++k)
    if (x[k] > x[am]) am = k;
  return am;
}

struct CeRow { float m, s; };
// softmax statistics of x
__device__ __forceinline__ CeRow ce_row(const float* x, int K) {
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, x[k]);
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(x[k] - m);
  return {m, s};
}
// cross entropy: w * -log softmax(x)[t], and its gradient by x[k].  m - x[t] comes first: it is exact for logits of like size, where
// (log s + m) - x[t] rounds log s to the spacing of m (1e-3 for logits near 1e4) before the large parts cancel.
__device__ __forceinline__ float ce_loss(const float* x, int t, float w, CeRow r) { return w * (logf(r.s) + (r.m - x[t])); }
__device__ __forceinline__ float ce_grad(const float* x, int k, int t, float w, CeRow r) { return w * (expf(x[k] - r.m) / r.s - (k == t ? 1.f : 0.f)); }

struct FocalRow { Soft1 a; float m2, s2; };                // both softmaxes' statistics: they do not depend on the target
__device__ __forceinline__ FocalRow focal_row(const float* x, int K, float lo, float hi) {
  const Soft1 a = soft1(x, K, lo, hi);
  float m2 = -INFINITY;
  for (int k = 0; k < K; ++k) m2 = fmaxf(m2, clampf(p1_of(x, k, a, lo, hi), lo, hi));
  float s2 = 0.f;
  for (int k = 0; k < K; ++k) s2 += expf(clampf(p1_of(x, k, a, lo, hi), lo, hi) - m2);
  return {a, m2, s2};
}
struct FocalTarget { float l, c, dot; };                   // the loss w (1-pt)^gamma * -log(eps + pt), c = dl/dpt * pt, dot = sum_j g1_j p1_j
__device__ __forceinline__ FocalTarget focal_target(const float* x, int K, int t, float w, FocalRow r, float gamma, float eps, float lo, float hi) {
  const float pt = expf(clampf(p1_of(x, t, r.a, lo, hi), lo, hi) - r.m2) / r.s2;
  const float om = 1.f - pt, nll = -logf(eps + pt);
  const float fg = powf(om, gamma);
  // dl/dpt = -gamma (1-pt)^(gamma-1) nll - (1-pt)^gamma / (eps + pt)
  const float dpt = w * (-gamma * powf(om, gamma - 1.f) * nll - fg / (eps + pt));
  const float c = dpt * pt;
  // through softmax 2 and clamp 2: g1_j = dpt * pt * (delta_tj - p2_j) * [lo <= p1_j <= hi];  dot = sum_j g1_j p1_j
  float dot = 0.f;
  for (int j = 0; j < K; ++j) {
    const float p1 = p1_of(x, j, r.a, lo, hi);
    const float p2 = expf(clampf(p1, lo, hi) - r.m2) / r.s2;
    const float g1 = (p1 >= lo && p1 <= hi) ? c * ((j == t ? 1.f : 0.f) - p2) : 0.f;
    dot += g1 * p1;
  }
  return {w * fg * nll, c, dot};
}
__device__ __forceinline__ float focal_grad(const float* x, int k, int t, FocalRow r, FocalTarget f, float lo, float hi) {
  const float p1 = p1_of(x, k, r.a, lo, hi);
  const float p2 = expf(clampf(p1, lo, hi) - r.m2) / r.s2;
  const float g1 = (p1 >= lo && p1 <= hi) ? f.c * ((k == t ? 1.f : 0.f) - p2) : 0.f;
  return (x[k] >= lo && x[k] <= hi) ? p1 * (g1 - f.dot) : 0.f;
}

// The end of both kernels: a fixed tree over the 256 threads' (loss, denominator, correct) sums, the division of the gradient rows by the
// mean's denominator, the reduced loss and the meter.
// 'mean' with a zero denominator (every row ignored, or zero class weights on all the others): the loss is 0/0 = NaN for both kinds, and the
// gradient is what the references return -- torch's cross entropy leaves the ignored rows' zeros alone and divides the others (NaN); the
// focal reference divides every row, ignored ones too (NaN), except the logits outside its clamp, whose gradient the clamp has masked to 0.
struct LossRows { const float* logits; const long long* ta; const long long* tb; long long ignore_index; float lo, hi; int kind; };   // tb may be null
__device__ __forceinline__ void loss_finish(float (*red)[256], float lsum, float wsum, float correct, float* loss_out, float* dlogits, float* meter,
                                            int B, int K, int reduction, LossRows q) {
  const int tid = threadIdx.x;
  red[0][tid] = lsum; red[1][tid] = wsum; red[2][tid] = correct;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  const float den = reduction == 0 ? red[1][0] : 1.f;      // 'mean': sum over not-ignored samples of their weight
  const float loss = red[0][0] / den;
  if (den != 0.f) {
    for (int b = tid; b < B; b += 256) {
      float* dx = dlogits + (size_t)b * K;
      for (int k = 0; k < K; ++k) dx[k] /= den;
    }
  } else {
    for (int b = tid; b < B; b += 256) {
      const float* x = q.logits + (size_t)b * K;
      float* dx = dlogits + (size_t)b * K;
      if (q.kind == 0 && (q.ta[b] == q.ignore_index || (q.tb != nullptr && q.tb[b] == q.ignore_index))) continue;
      for (int k = 0; k < K; ++k)
        if (q.kind == 0 || (x[k] >= q.lo && x[k] <= q.hi)) dx[k] /= den;
    }
  }
  if (tid == 0) {
    if (reduction != 2) loss_out[0] = loss;
    if (meter != nullptr) {                                // train.py:327-328: running_loss += loss * B; num_acc += correct
      // 'none': loss is already the batch sum (den = 1), so the meter takes it as is -- the mean's loss * B of an unweighted batch
      meter[0] += reduction == 2 ? red[0][0] : loss * (float)B;
      meter[1] += red[2][0];
      meter[2] += (float)B;
    }
  }
}

__global__ __launch_bounds__(256) void loss_kernel(LossArgs p) {
  __shared__ float red[3][256];
  const int tid = threadIdx.x, K = p.K;
  const float lo = p.eps, hi = p.hi;
  float lsum = 0.f, wsum = 0.f, correct = 0.f;
  for (int b = tid; b < p.B; b += 256) {
    const float* x = p.logits + (size_t)b * K;
    float* dx = p.dlogits + (size_t)b * K;
    const long long tg = p.target[b];
    const bool ign = tg == p.ignore_index;
    if (!ign && (tg < 0 || tg >= (long long)K)) {         // a bad row: not a class, nothing is read at it
      for (int k = 0; k < K; ++k) dx[k] = NAN;
      if (p.reduction == 2) p.loss[b] = NAN;
      lsum += NAN;
      continue;
    }
    const int t = ign ? 0 : (int)tg;
    const float w = p.weights != nullptr ? p.weights[t] : 1.f;
    if (!ign && argmax_row(x, K) == t) correct += 1.f;
    if (ign) {
      for (int k = 0; k < K; ++k) dx[k] = 0.f;
      if (p.reduction == 2) p.loss[b] = 0.f;             // 'none': an ignored row's loss is masked to zero (focal_loss.py:108)
      continue;
    }
    wsum += w;
    if (p.kind == 0) {                                    // cross entropy: -log softmax(x)[t]
      const CeRow r = ce_row(x, K);
      const float l = ce_loss(x, t, w, r);
      lsum += l;
      if (p.reduction == 2) p.loss[b] = l;
      for (int k = 0; k < K; ++k) dx[k] = ce_grad(x, k, t, w, r);
      continue;
    }
    const FocalRow r = focal_row(x, K, lo, hi);
    const FocalTarget f = focal_target(x, K, t, w, r, p.gamma, p.eps, lo, hi);
    lsum += f.l;
    if (p.reduction == 2) p.loss[b] = f.l;                // 'none' (focal_loss.py:118): the per-sample vector, dlogits = its rows' own gradients
    for (int k = 0; k < K; ++k) dx[k] = focal_grad(x, k, t, r, f, lo, hi);
  }
  loss_finish(red, lsum, wsum, correct, p.loss, p.dlogits, p.meter, p.B, K, p.reduction, LossRows{p.logits, p.target, nullptr, p.ignore_index, lo, hi, p.kind});
}

// ---- mixed targets (Mixup / CutMix) and label smoothing --------------------------------------------------------------------------------
// l_i = lam_i l(x_i, a_i) + (1 - lam_i) l(x_i, b_i), l = the per-sample loss above, class weight included; for cross entropy with smoothing e
//   l(x, t) = (1 - e) w_t (-log p_t) + (e / K) sum_k w_k (-log p_k)      (torch's label_smoothing rule for class-index targets).
// A side whose coefficient is zero is not evaluated, so lam = 1 (or no partner at all) with e = 0 runs exactly the operations of loss_kernel
// and returns its bits.  'mean' divides by sum_i (lam_i w_{a_i} + (1 - lam_i) w_{b_i}) over the rows that are not ignored; a row is ignored
// when a_i or b_i is ignore_index, and bad (see the top of the file) when it is not ignored and a_i or b_i is no class, whatever lam_i is;
// the meter's accuracy counts argmax == the dominant label (a_i when lam_i >= 0.5, else b_i).
struct LossMixedArgs {
  const float* logits; const long long* target_a; const long long* target_b; const float* lam; const float* weights;
  float* loss; float* dlogits; float* meter;
  int B, K, kind, reduction;
  float gamma, eps, hi, smoothing;
  long long ignore_index;
};

__global__ __launch_bounds__(256) void loss_mixed_kernel(LossMixedArgs p) {
  __shared__ float red[3][256];
  const int tid = threadIdx.x, K = p.K;
  const float lo = p.eps, hi = p.hi;
  const float e = p.smoothing, keep = 1.f - e, ek = e / (float)K;
  float lsum = 0.f, wsum = 0.f, correct = 0.f;
  for (int b = tid; b < p.B; b += 256) {
    const float* x = p.logits + (size_t)b * K;
    float* dx = p.dlogits + (size_t)b * K;
    const long long ta = p.target_a[b], tb = p.target_b != nullptr ? p.target_b[b] : ta;
    const bool ign = ta == p.ignore_index || tb == p.ignore_index;
    if (ign) {
      for (int k = 0; k < K; ++k) dx[k] = 0.f;
      if (p.reduction == 2) p.loss[b] = 0.f;
      continue;
    }
    if (ta < 0 || ta >= (long long)K || tb < 0 || tb >= (long long)K) {   // a bad row: either label is not a class, nothing is read at it
      for (int k = 0; k < K; ++k) dx[k] = NAN;
      if (p.reduction == 2) p.loss[b] = NAN;
      lsum += NAN;
      continue;
    }
    const float ca = p.lam != nullptr ? p.lam[b] : 1.f, cb = 1.f - ca;
    const bool sa = ca != 0.f, sb = cb != 0.f;            // the sides that count
    const int t[2] = {(int)ta, (int)tb};
    const float w[2] = {p.weights != nullptr ? p.weights[t[0]] : 1.f, p.weights != nullptr ? p.weights[t[1]] : 1.f};
    if (argmax_row(x, K) == (ca >= 0.5f ? t[0] : t[1])) correct += 1.f;
    wsum += sb ? (sa ? ca * w[0] + cb * w[1] : cb * w[1]) : ca * w[0];
    float l;
    if (p.kind == 0) {
      const CeRow r = ce_row(x, K);
      float la = sa ? ce_loss(x, t[0], w[0], r) : 0.f, lb = sb ? ce_loss(x, t[1], w[1], r) : 0.f;
      float wall = 0.f;                                     // sum_k w_k, and the smoothing term (e / K) sum_k w_k (-log p_k), the same for both sides
      if (e != 0.f) {
        float u = 0.f;
        for (int k = 0; k < K; ++k) {
          const float wk = p.weights != nullptr ? p.weights[k] : 1.f;
          wall += wk;
          u += ce_loss(x, k, wk, r);
        }
        la = keep * la + ek * u;
        lb = keep * lb + ek * u;
      }
      l = sb ? (sa ? ca * la + cb * lb : cb * lb) : ca * la;
      for (int k = 0; k < K; ++k) {
        float ga = sa ? ce_grad(x, k, t[0], w[0], r) : 0.f, gb = sb ? ce_grad(x, k, t[1], w[1], r) : 0.f;
        if (e != 0.f) {                                   // d/dx_k sum_j w_j (-log p_j) = p_k sum_j w_j - w_k
          const float wk = p.weights != nullptr ? p.weights[k] : 1.f;
          const float gu = ek * (expf(x[k] - r.m) / r.s * wall - wk);
          ga = keep * ga + gu;
          gb = keep * gb + gu;
        }
        dx[k] = sb ? (sa ? ca * ga + cb * gb : cb * gb) : ca * ga;
      }
    } else {
      const FocalRow r = focal_row(x, K, lo, hi);
      FocalTarget fa = {0.f, 0.f, 0.f}, fb = {0.f, 0.f, 0.f};
      if (sa) fa = focal_target(x, K, t[0], w[0], r, p.gamma, p.eps, lo, hi);
      if (sb) fb = focal_target(x, K, t[1], w[1], r, p.gamma, p.eps, lo, hi);
      l = sb ? (sa ? ca * fa.l + cb * fb.l : cb * fb.l) : ca * fa.l;
      for (int k = 0; k < K; ++k) {
        const float ga = sa ? focal_grad(x, k, t[0], r, fa, lo, hi) : 0.f, gb = sb ? focal_grad(x, k, t[1], r, fb, lo, hi) : 0.f;
        dx[k] = sb ? (sa ? ca * ga + cb * gb : cb * gb) : ca * ga;
      }
    }
    lsum += l;
    if (p.reduction == 2) p.loss[b] = l;
  }
  loss_finish(red, lsum, wsum, correct, p.loss, p.dlogits, p.meter, p.B, K, p.reduction, LossRows{p.logits, p.target_a, p.target_b, p.ignore_index, lo, hi, p.kind});
}

}  // namespace gvk

extern "C" int gvk_loss_fwd_bwd(const gvk_loss_desc* d, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(d && d->logits && d->target && d->loss && d->dlogits, "gvk_loss_fwd_bwd: null pointer");
  GVK_REQUIRE(d->B > 0 && d->K > 1 && d->K <= 4096, "gvk_loss_fwd_bwd: B=%d K=%d (K = 1, the sigmoid branch, is not built)", d->B, d->K);
  GVK_REQUIRE(d->kind == GVK_LOSS_CE || d->kind == GVK_LOSS_FOCAL, "gvk_loss_fwd_bwd: unknown kind %d", d->kind);
  GVK_REQUIRE(d->reduction >= 0 && d->reduction <= 2, "gvk_loss_fwd_bwd: reduction must be 0 (mean), 1 (sum) or 2 (none: loss receives B values)");
  LossArgs a{d->logits, (const long long*)d->target, d->weights, d->loss, d->dlogits, d->meter, d->B, d->K, d->kind, d->reduction,
             d->gamma, d->eps, 1.f - d->eps, (long long)d->ignore_index};
  GVK_LAUNCH(loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("loss_fwd_bwd");
}

extern "C" int gvk_loss_mixed_fwd_bwd(const gvk_loss_mixed_desc* d, void* stream) {
  using namespace gvk;
  GVK_REQUIRE(d && d->logits && d->target_a && d->loss && d->dlogits, "gvk_loss_mixed_fwd_bwd: null pointer");
  GVK_REQUIRE((d->target_b == nullptr) == (d->lam == nullptr), "gvk_loss_mixed_fwd_bwd: target_b and lam come together (both NULL: no partner, lam = 1)");
  GVK_REQUIRE(d->B > 0 && d->K > 1 && d->K <= 4096, "gvk_loss_mixed_fwd_bwd: B=%d K=%d (K = 1, the sigmoid branch, is not built)", d->B, d->K);
  GVK_REQUIRE(d->kind == GVK_LOSS_CE || d->kind == GVK_LOSS_FOCAL, "gvk_loss_mixed_fwd_bwd: unknown kind %d", d->kind);
  GVK_REQUIRE(d->reduction >= 0 && d->reduction <= 2, "gvk_loss_mixed_fwd_bwd: reduction must be 0 (mean), 1 (sum) or 2 (none: loss receives B values)");
  GVK_REQUIRE(d->smoothing >= 0.f && d->smoothing <= 1.f, "gvk_loss_mixed_fwd_bwd: smoothing %g is outside [0, 1]", (double)d->smoothing);
  GVK_REQUIRE(d->kind == GVK_LOSS_CE || d->smoothing == 0.f, "gvk_loss_mixed_fwd_bwd: label smoothing is built for the cross entropy only");
  LossMixedArgs a{d->logits, (const long long*)d->target_a, (const long long*)d->target_b, d->lam, d->weights, d->loss, d->dlogits, d->meter,
                  d->B, d->K, d->kind, d->reduction, d->gamma, d->eps, 1.f - d->eps, d->smoothing, (long long)d->ignore_index};
  GVK_LAUNCH(loss_mixed_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("loss_mixed_fwd_bwd");
}
