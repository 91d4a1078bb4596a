/* gaviko_hip.h -- C-ABI of libgaviko_hip.so: the MI355X (gfx950) kernels behind GAViKO's 3D-ViT hot path.
 *
 * Boundary contract
 *   - plain C: device pointers + sizes + a hipStream_t passed as void*; no torch / C++ types.
 *   - every entry point enqueues on `stream` and returns immediately: 0 = ok, <0 = error
 *     (gvk_last_error() holds the message).  No allocation, no synchronisation, graph-capture safe.
 *   - "bf16" = raw uint16 storage of bfloat16.  Row-major everywhere.
 *   - activation matrices [M][ld] must be allocated with at least round_up(M,128) rows (the MFMA tiles read
 *     whole 128-row panels; rows >= M are computed but never stored).
 *
 * What each entry point replaces in the reference (implicit ATen dispatches):
 *   the reference has no native code -- citations are to the Python call sites, /root/reference/src/.
 */
#ifndef GAVIKO_HIP_H
#define GAVIKO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* gvk_last_error(void);
/* returns 950 when the code object loaded on the current device is gfx950, else <0 */
int gvk_device_check(void);
int gvk_abi_version(void);   /* 14 */

/* ------------------------------------------------------------------ launch plans
 * The reference drives its step from the Python interpreter (train.py:296-319: one autograd node per op).  Here one
 * training step is ~670 launches on three streams; a plan records them once (kernel, grid, by-value arguments, stream,
 * and the event record/wait edges between streams) and gvk_plan_replay re-issues them from a single C loop.
 * Recording is per host thread: between gvk_plan_begin and gvk_plan_end every gvk_* launch made by that thread both
 * executes and is appended to the plan.  Pointers are baked in: replay is valid while the buffers passed at record
 * time stay allocated (the engine's static workspace).  Events used for cross-stream edges inside a plan must come
 * from gvk_plan_event_record.  gvk_plan_end returns the plan id (>= 0).                                              */
int gvk_plan_begin(void);
int gvk_plan_end(void);
int gvk_plan_abort(void);
int gvk_plan_size(int plan);                       /* number of recorded nodes */
int gvk_plan_replay(int plan);
int gvk_plan_free(int plan);
int gvk_plan_event_record(void* stream);           /* -> event id within the plan being recorded */
int gvk_plan_event_wait(void* stream, int event);
/* gvk_plan_event_record with the system-scope fence kept (events that peer devices' reads are ordered behind: all-reduce buckets) */
int gvk_plan_event_record_fenced(void* stream);
/* issued immediately (not recorded): `stream` waits for event `event` of plan `plan` as recorded by its most recent replay */
int gvk_plan_event_stream_wait(int plan, int event, void* stream);
/* measurement: milliseconds between two events of a replayed plan.  Events carry timestamps only in plans recorded after
 * gvk_plan_set_timing(1) (or with GAVIKO_HIP_PLAN_TIMING set in the environment); bench.py brackets the GEMM launches
 * of an instrumented copy of the step this way, so the kernels are timed inside the real three-stream schedule. */
int gvk_plan_set_timing(int on);
int gvk_plan_event_elapsed(int plan, int e0, int e1, float* ms);
/* small stream-ordered utilities the step needs between kernels (recorded into a plan like any launch) */
/* byte fill by a fill kernel, not a runtime memset: the low byte of `value`; ptr 16-byte aligned, bytes a multiple of 4; 0 does nothing */
int gvk_memset_async(void* ptr, int value, size_t bytes, void* stream);
int gvk_seed_advance(void* seed_u64, uint64_t inc, void* stream);   /* device-side dropout epoch += inc */
int gvk_scale_f32(float* x, float alpha, long n, void* stream);

/* ------------------------------------------------------------------ bf16 MFMA GEMM  Y = A . W^T (+ epilogue)
 * A [M][lda] bf16 (K contiguous), W [N][ldw] bf16 (K contiguous, i.e. nn.Linear.weight layout), fp32 accumulate.
 * Replaces every nn.Linear / Conv3d-as-GEMM on the path:
 *   model/vision_transformer.py:62 (to_qkv), :72 (to_out), :31,34 (MLP fc1/fc2), :150 (conv_proj) and their
 *   autograd dgrads (dX = dY . W, expressed as NT with the pre-transposed frozen weight). */
enum gvk_epilogue {
  GVK_EPI_STORE_BF16 = 0,     /* out0 bf16 [M][ldo] = acc (+bias)                                                */
  GVK_EPI_BIAS_RES_F32 = 1,   /* out0 f32  = acc + bias[n] + res[m][n]  (residual add; res may alias out0)        */
  GVK_EPI_BIAS_GELU_BF16 = 2, /* out0 bf16 = acc + bias (pre-activation, may be NULL); out1 bf16 = erf-GELU(out0) */
  GVK_EPI_PATCH_F32 = 3,      /* out0 f32 [(m/rows_in)*rows_out + row_off + m%rows_in][n] = acc + bias + pos[m%rows_in][n];
                                 out1 f32 [m][n] (may be NULL) = same value (GAViKO local stream)                 */
  GVK_EPI_GELU_BWD_BF16 = 4,  /* out0 bf16 = acc * GELU'(aux bf16 [m][n])   (fc2 dgrad fused with GELU backward)   */
  GVK_EPI_STORE_F32 = 5,      /* out0 f32  = acc (+bias)                                                          */
  GVK_EPI_BIAS_RES_F32_BF16 = 6, /* as 1, and out1 bf16 [M][ldo] = same value rounded                             */
  GVK_EPI_BIAS_RELU_BF16 = 7, /* out0 bf16 = max(acc + bias, 0)          (AdaptFormer down-projection, adaptformer.py:63-64)   */
  GVK_EPI_RELU_BWD_BF16 = 8   /* out0 bf16 = acc * (aux bf16 [m][n] > 0) (dgrad through that ReLU)                              */
};

typedef struct gvk_gemm_desc {
  const void* a;      /* bf16 [>=round_up(M,128)][lda] */
  const void* w;      /* bf16 [N][ldw] */
  void* out0;
  void* out1;
  const float* bias;  /* [N] or NULL */
  const float* res;   /* f32 [M][ldres] or NULL */
  const void* aux;    /* bf16 [M][ldaux] or NULL */
  const float* pos;   /* f32 [rows_in][N] or NULL */
  const void* seed_ptr; /* device uint64 dropout epoch (drop_p > 0) */
  int32_t M, N, K;
  int32_t lda, ldw, ldo, ldres, ldaux;
  int32_t epilogue;
  int32_t rows_in, rows_out, row_off; /* GVK_EPI_PATCH_F32 only */
  int32_t tile;       /* 0 = auto, else BM*1000+BN (128128, 128064, 64064, 64128); 3128128 / 3064128 = 128x128 / 64x128 with three LDS stages; 3096128 = 96x128 with three stages;;
                         256256 = eight waves on a 256x256 tile (STORE_BF16, BIAS_GELU_BF16, GELU_BWD_BF16 only);
                         8256256 / 7256256 = the eight-phase 256x256 kernel (gemm8p_bf16.hip: two wave groups one barrier apart, counted
                         vmcnt), LDS-DMA issued in the load sections / inside the MFMA clusters; epilogues 0, 1, 2, 4, 5, N % 256 == 0, K >= 128 */
  float drop_p;       /* nn.Dropout behind the Linear (vision_transformer.py:32-34,54), epilogues 1, 2 (on out1), 4: the value at
                         (m, n) is multiplied by mask(seed + *seed_ptr, m*N + n) / (1 - drop_p); 0 = off */
  uint64_t seed;
  int32_t scale_cols; /* GVK_EPI_STORE_BF16 (bf16 entry point) only: columns n < scale_cols (a multiple of 8) are multiplied by col_scale in fp32 */
  float col_scale;    /* before the ONE rounding to bf16 -- the q block of a qkv projection leaves the GEMM as q * scale * log2(e), the form
                         the bf16 attention kernels take (gvk_attention_desc); 0 columns = off */
  /* LayerNorm folded into its consumer (GVK_EPI_STORE_BF16, bf16 entry point): a = the RAW rows x as bf16, w = gamma o W; with ln_mean /
     ln_rstd f32 [M] and ln_c1 f32 [N] = row sums of w (of its bf16 values) the epilogue stores rstd[m]*(acc - mean[m]*c1[n]) + bias[n],
     bias[n] = sum_c beta[c] W[n][c] -- LayerNorm(x) . W^T (vision_transformer.py:49,61-62) without the LayerNorm launch.  NULL = off */
  const float* ln_mean; const float* ln_rstd; const float* ln_c1;
  /* GVK_EPI_BIAS_RES_F32_BF16: also write per-row partial (sum, sum of squares) of the fp32 output, f32 [N / 64][M][2] (64-column groups
     of the 128-wide tiles); gvk_prompt_up_fix_stats turns them into the mean / rstd the folded consumer reads.  NULL = off.
     The partials are taken of (x - stat_pivot[m]), stat_pivot f32 [M] = any per-row estimate of the row mean (the engine passes the
     mean of the residual row, which its LayerNorm has just computed): shifted sums do not cancel when |mean| >> std, which the plain
     E[x^2] - mean^2 form does.  stat_pivot NULL = pivot 0 */
  float* stat_part;
  const float* stat_pivot;
  /* Row PANELS at a stride (bf16 entry point; 0 = off): the launch covers m_panels row tiles whose first rows are 0, m_stride, 2 m_stride, ...
     (the first rows of every sample of a [B][T][.] token tensor: m_stride = T) instead of the contiguous rows 0 .. M-1; M stays the
     number of rows the operands have (rows >= M are not stored).  Only rows of the panels are read and written.  What it is for: a
     product whose other rows are never consumed -- the last layer's MLP when the head pools the first rows of every sample
     (gaviko.py:316), the first layer's qkv dgrad when only the prompt rows of the input carry a trainable tensor.  Tile: one of the
     4-wave kernels (tile = 0 picks 64 x 128 with three stages), m_stride >= the tile's rows, (m_panels - 1) * m_stride + tile rows <= the padded M */
  int32_t m_panels, m_stride;
  /* with m_panels: cut every tile's K loop into pieces over otherwise idle CUs (a few 64-row tiles run at the latency of one workgroup's
     loop); the pieces are summed in a fixed order by the workgroup that arrives last (no float atomics, bitwise reproducible).
     splitk_ws: 256-byte aligned device memory, >= 1 KiB + tiles * 8 * 32 KiB, its first KiB ZERO at allocation (ticket words, left zero);
     launches that share it must be ordered by their stream.  NULL = one workgroup per tile */
  void* splitk_ws; uint64_t splitk_ws_bytes;
  /* pieces per tile (2..8) when splitk_ws is given; 0 = as many as keep the launch within one round of the chip.  Also: tile = 2128128 runs a
     FULL launch (no panels) of <= 256 tiles of 128 x 128 this way -- two pieces of a K >= 2304 loop on two workgroups that share a CU
     (measured: no faster than one three-stage workgroup per tile; the engine does not use it) */
  int32_t ksplit;
  /* (bf16 entry point, no dropout) the GELU derivative is computed ONCE, where its exponential is computed anyway: with aux_is_grad = 1
     GVK_EPI_BIAS_GELU_BF16 stores out0 = bf16 GELU'(acc + bias) instead of the pre-activation, and GVK_EPI_GELU_BWD_BF16 reads aux as that
     derivative (out0 = acc * aux).  A caller sets it on both GEMMs of an MLP (vision_transformer.py:31-34 and its autograd) or on neither */
  int32_t aux_is_grad;
} gvk_gemm_desc;
int gvk_gemm_nt_bf16(const gvk_gemm_desc* d, void* stream);
/* number of 64-column groups gvk_gemm_desc.stat_part is indexed by for an N-column output */
int gvk_gemm_stat_parts(int N);

/* ------------------------------------------------------------------ fp32 compute path
 * BASELINE cfg4 (adaptformer / melo) runs the reference in fp32 with a 1e-5 tolerance, which bf16 MFMA operands cannot
 * meet.  These entry points mirror their bf16 namesakes argument for argument -- same descriptor, same epilogue table,
 * same layouts -- with every 16-bit slot (A, W, bf16 outputs, aux) carrying float.  GELU is the exact erf form.
 * gvk_gemm_nt_f32: v_mfma_f32_16x16x4_f32 (exact fp32 products), N % 64 == 0, K % 16 == 0.
 * fp32 attention is gvk_attention_fwd / gvk_attention_bwd with gvk_attention_desc.f32 = 1 (below). */
int gvk_gemm_nt_f32(const gvk_gemm_desc* d, void* stream);
int gvk_patchify_f32(const float* img, float* out, int B, int D, int H, int W, int pd, int ph, int pw, void* stream);
int gvk_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
int gvk_transpose_bf16(const void* in, void* out, int rows, int cols, void* stream);   /* operand transposes of the unfrozen-backbone wgrad GEMMs */
int gvk_copy_f32_strided(const float* in, float* out, int M, int C, int ld_in, void* stream);   /* out[M][C] = in[M][ld_in] cols 0..C */
/* stream-ordered device-to-device copy: a copy kernel, not a runtime memcpy, recorded into a launch plan like any launch.
 * Both pointers 16-byte aligned, bytes a multiple of 4; bytes == 0 does nothing. */
int gvk_copy_async(void* dst, const void* src, size_t bytes, void* stream);

/* ------------------------------------------------------------------ casts / layout
 * fp32 -> bf16 copy of a [rows][cols] matrix (weights -> MFMA operand form), optionally transposed
 * (out [cols][rows]) for the dgrad operand of frozen weights. */
int gvk_cast_f32_bf16(const float* in, void* out, int64_t n, void* stream);
int gvk_transpose_cast_f32_bf16(const float* in, void* out, int rows, int cols, void* stream);
/* Split-bf16 packing of a narrow fp32 operand into 3 ca + 2 spare K columns (from col0) of a bf16 GEMM operand dst [rows][ld_dst]:
 * x = hi + lo (hi = bf16(x), lo = bf16(x - hi)); activation side (weight_side 0) writes [a_hi | a_lo | a_hi], weight side writes
 * [w_hi | w_hi | w_lo | b_hi | b_lo] (b f32 [rows] or NULL; it meets two constant-1 columns of the activation operand).  The GPA
 * up-projection (gaviko.py:187, x + proj_up(.)) then rides the MLP's second Linear (vision_transformer.py:34) as K-concatenation,
 * A' = [act | lat_hi | lat_lo | lat_hi | 1 | 1], W' = [W_fc2 | Wup_hi | Wup_hi | Wup_lo | b_hi | b_lo], at ~2^-16 relative accuracy. */
int gvk_pack_split_bf16(const float* a, int ca, const float* b, void* dst, int ld_dst, int col0, int rows, int weight_side, void* stream);
/* im2col of non-overlapping 3-D patches, fp32 volume -> bf16 rows [B*n_patches][pd*ph*pw]
 * (K order (kd,kh,kw) == Conv3d weight.flatten(1); vision_transformer.py:126-128,150-151). */
int gvk_patchify_bf16(const float* img, void* out, int B, int D, int H, int W, int pd, int ph, int pw, void* stream);


/* ------------------------------------------------------------------ LayerNorm (eps 1e-5; vision_transformer.py:30,49,77)
 * fwd: x f32 [M][C] -> y bf16 [M][C] (MFMA operand) and/or y32 f32; saves mean/rstd f32 [M] (either may be NULL). */
int gvk_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* y_f32,
                      float* mean, float* rstd, int M, int C, float eps, void* stream);
/* gvk_layernorm_fwd (bf16 output) with the GPA prompt fix of the previous layer applied on the way in: rows with (m % T) < P first receive
 * x[m] += (enh[m / T][m % T] - lat[m]) . wup^T (wup f32 [C][L]; gaviko.py:183-187 when the plain-latent part rode the MLP GEMM) and are
 * written back; then every row is normalised.  Replaces gvk_prompt_up_fix + gvk_layernorm_fwd at a layer boundary. */
int gvk_layernorm_fwd_fix(float* x, const float* gamma, const float* beta, void* y_bf16, float* mean, float* rstd, int M, int C, float eps,
                          const float* enh, const float* lat, const float* wup, int T, int P, int L, void* stream);
/* affine gradients of a trainable LayerNorm: dgamma[c] += sum_m dy*xhat, dbeta[c] += sum_m dy (accumulate=0 overwrites).
 * scratch: f32 [2*64*C]. */
int gvk_layernorm_bwd_affine(const float* dy, const float* x, const float* mean, const float* rstd, float* dgamma,
                             float* dbeta, float* scratch, int M, int C, int accumulate, void* stream);

/* LayerNorm with a fused rank-L projection of the rows it already holds (L = 20 = configs/gaviko.yaml prompt_latent_dim):
 *   fwd_proj:  y_bf16 = LN(x) as gvk_layernorm_fwd, and   proj->y = act(x . W^T + bias)        of the RAW input rows
 *              (gaviko.py:155-156: GPA proj_down + QuickGELU of the post-attention stream; proj->z = pre-activation);
 *   bwd (gvk_ln_bwd_desc.proj):  dx as without it, and    proj->y = dx . W                      of the OUTPUT rows
 *              (autograd of gaviko.py:187 proj_up: the next-lower layer's dcomb = dG . W_up).
 * w_layout 0: w [L][C]; 1: w [C][L].  Covers L in {4, 8, 16, 20} and 128 <= C <= 1024; otherwise use gvk_skinny_down. */
typedef struct gvk_rowproj_desc {
  const float* w; const float* bias;       /* bias [L] or NULL */
  float* y; float* z;                      /* y [M][L]; z [M][L] pre-activation or NULL */
  void* y_split;                           /* optional: split-bf16 copy [hi | lo | hi] of y (gvk_pack_split_bf16, activation side) into columns
                                              col_split .. col_split + 3L - 1 of a bf16 [M][ld_split] GEMM operand */
  int32_t L, w_layout, act;                /* act: 0 none, 1 QuickGELU */
  int32_t ld_split, col_split;
} gvk_rowproj_desc;
int gvk_layernorm_fwd_proj(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean, float* rstd,
                           int M, int C, float eps, const gvk_rowproj_desc* proj, void* stream);
/* bwd (input gradient only -- frozen affine): dx = dres + LN'(dy) over f32 [M][C] rows; dres may be NULL; dx_bf16 (optional) = bf16 copy of dx.
 * Three optional features:
 *   dy_bf16 = 1: dy is bf16 [M][C] -- the form a dgrad GEMM with the STORE_BF16 epilogue leaves it in (fc1 / qkv dgrad of a frozen backbone:
 *     half the bytes written by the GEMM and read here); 0: dy is f32;
 *   rows_per_group > 0: a row SUBSET, rows g * group_stride + r, r < rows_per_group, g < groups, of every operand (the first rows of every
 *     sample; must fit M); the other rows are neither read nor written.  0: all M rows;
 *   proj != NULL: the rank-L projection proj->y = dx . W rides along (see gvk_rowproj_desc above); all rows only (rows_per_group = 0). */
typedef struct gvk_ln_bwd_desc {
  const void* dy; const float* x; const float* mean; const float* rstd; const float* gamma; const float* dres;
  float* dx; void* dx_bf16;
  const gvk_rowproj_desc* proj;
  int32_t M, C, groups, rows_per_group, group_stride, dy_bf16;
} gvk_ln_bwd_desc;
int gvk_layernorm_bwd(const gvk_ln_bwd_desc* d, void* stream);
/* LayerNorm backward fused with a rank-L update of the same rows:  dx = dres + LN'(dy; x, mean, rstd, gamma) + lat . W^T  (+ bf16 copy).
 * Replaces gvk_layernorm_bwd followed by gvk_skinny_up(accumulate) on the backbone stream: the autograd of gaviko.py:304 (the MLP block's
 * LayerNorm) and of gaviko.py:155 (GPA's proj_down of the global tokens: dG1 += dzx . W_d) in one pass.  lat f32 [M][L]; w_layout 0: W [C][L],
 * 1: W [L][C].  Covers L = 20, C in {192, 768, 1024}. */
int gvk_layernorm_bwd_up(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* dres,
                         float* dx, void* dx_bf16, const float* lat, const float* w, int w_layout, int M, int C, int L, void* stream);

/* ------------------------------------------------------------------ multi-head self-attention, head dim 64
 * One descriptor, one forward and one backward entry point for every form of the flash-style attention (vision_transformer.py:62-71).
 * qkv bf16 [B*T (padded)][ld_qkv]: columns [q' | k | v], each (head, 64) -- the to_qkv output (vision_transformer.py:62-63) with the q
 * block PRE-SCALED: q' = q * scale * log2(e), multiplied in fp32 before the one rounding to bf16.  gvk_gemm_nt_bf16 does it in the
 * projection's epilogue (gvk_gemm_desc.scale_cols = H*64, col_scale = scale * log2(e)); gvk_qkv_prescale_bf16 converts a raw qkv buffer
 * in place.  The forward and both backward passes then read bit-identical score operands (P of the backward is recomputed against the
 * forward's lse) and no kernel spends a multiply per score.  scale = dim_head^-0.5 (vision_transformer.py:47,65).
 *   fwd: reads qkv; writes out bf16 [B*T][ld_out] in 'b n (h d)' order (vision_transformer.py:71) and lse f32 [B][H][T] = log sum_j
 *     exp(scale * q.k_j) (natural log), saved for the backward.  dout, delta, dqkv and need_rows are ignored; ws must be NULL.
 *   bwd: reads qkv, out (for delta = rowsum(dout * out)), dout, lse; writes dqkv bf16 [B*T][ld_qkv] = [dq | dk | dv] in the qkv layout --
 *     gradients of the UNSCALED q, k, v (what the to_qkv dgrad consumes) -- and delta f32 [B][H][T] (scratch).  Two passes, no atomics,
 *     bitwise reproducible.
 * ld_qkv >= 3*H*64, ld_out >= H*64, every row pitch a multiple of 16 bytes; a bf16 qkv tensor stays below 2 GiB.
 * Four optional features.  They exclude each other where stated: a contradictory descriptor is an error, never resolved by precedence.
 *   f32 = 1: every 16-bit slot (qkv, out, dout, dqkv) carries float and q is NOT pre-scaled (the kernels multiply by scale): the fp32
 *     compute path, products on the fp32 matrix cores, 1e-5 against float64.  Plain two-pass backward only: no need_rows, no ws;
 *   drop_p > 0: nn.Dropout(drop_p) on the attention probabilities (vision_transformer.py:52,68 -- live in training for the methods that
 *     do not freeze the backbone): softmax statistics of the undropped scores, out = (P * mask / (1 - drop_p)) . V; the backward
 *     regenerates mask(seed + *seed_ptr; b*H + head, query, key), the same function in both precisions.  0 <= drop_p < 1, T*T < 2^32.
 *     drop_p = 0: seed and seed_ptr are unused;
 *   need_rows > 0 (bwd, bf16, no dropout, no ws): only the FIRST need_rows tokens of every sample carry a consumer (the bottom layer of a
 *     frozen backbone: of its input only the prompt rows hold a trainable tensor, gaviko.py:540-548): dq, dk, dv of tokens < need_rows
 *     (rounded up to 128) are written -- the very bits the full call writes there, at whichever key tile -- the other rows of dqkv are
 *     left untouched; delta is complete.  0: all rows.  need_rows <= T;
 *   ws != NULL (bwd, bf16, no dropout, no need_rows): the ONE-PASS backward (round 5; ABI 10): five MFMA products per (query, key) block
 *     instead of seven and one exponential per score instead of two -- each workgroup owns dK / dV of its 128 keys and also forms dQ's
 *     share of those keys; the shares of a (batch, head)'s key blocks are summed by an ordered hand-off between the workgroups (fixed
 *     order per query tile: bitwise reproducible, no float atomics); delta is written by a small kernel in front.  ws: ws_bytes >=
 *     gvk_attention_bwd_ws_bytes(B, T, H) bytes, 256-byte aligned, ZERO at allocation (the kernel leaves its progress words zero); its
 *     layout depends on ws_bytes only, so ONE workspace sized for the longest sequence serves shorter ones too.  The int32 at byte
 *     gvk_attention_bwd_status_offset(ws_bytes) counts hand-off waits that ran into their bound and stays 0.  Calls that share a
 *     workspace must be ordered by their stream.  NULL: the two-pass backward. */
typedef struct gvk_attention_desc {
  const void* qkv; void* out; void* lse; const void* dout; void* delta; void* dqkv; const void* seed_ptr; void* ws;
  int32_t B, T, H, ld_qkv, ld_out, f32, need_rows;
  float scale, drop_p;
  uint64_t seed, ws_bytes;
} gvk_attention_desc;
int gvk_attention_fwd(const gvk_attention_desc* d, void* stream);
int gvk_attention_bwd(const gvk_attention_desc* d, void* stream);
size_t gvk_attention_bwd_ws_bytes(int B, int T, int H);
size_t gvk_attention_bwd_status_offset(size_t ws_bytes);
/* q block of a raw bf16 to_qkv output -> q * scale * log2(e), in place (rows = B*T) */
int gvk_qkv_prescale_bf16(void* qkv, int rows, int H, int ld_qkv, float scale, void* stream);
/* attention maps for explanations (csrc/attention_map.hip; what a forward hook on the reference's `attend` softmax sees,
 * vision_transformer.py:50,67): the probabilities P = softmax(scale q.k^T) of qkv / lse in the layout above, row-weighted and summed --
 *   out f32 [B][H][T]  out[b][h][j] = sum_{q0 <= i < q1} w[b][i] * P[b][h][i][j]   for j < T (nothing else is written)
 * w f32 [B][ld_w] (rows outside [q0, q1) are not read), 0 <= q0 < q1 <= T.  P is recomputed against lse, as the backward does.
 * Deterministic (no atomics).
 * gvk_rollout_step: one step of attention rollout with mean head fusion and residual weight 0.5 --
 *   r_out[b][j] = 0.5 * r_in[b][j] + (0.5 / H) * sum_h out[b][h][j]   (heads summed in order; r_out may alias r_in), r f32 [B][T]. */
int gvk_attention_colsum_bf16(const void* qkv, const float* lse, const float* w, int ld_w, float* out, int B, int T, int H, int ld_qkv,
                              int q0, int q1, void* stream);
int gvk_rollout_step(const float* r_in, const float* colsum, float* r_out, int B, int T, int H, void* stream);
/* class-specific attention relevance (gradient x attention; Chefer, Gur & Wolf 2021, "Generic Attention-model Explainability"): with
 * dO = the gradient of one logit with respect to the attention output (bf16 [B*T][ld_dctx], head h in columns 64 h .. 64 h + 63 -- the
 * backward sweep's dctx), dP[b][h][i][j] = dO[b][i][h][:] . v[b][j][h][:] is that logit's gradient with respect to P, and
 *   out f32 [B][H][T]  out[b][h][j] = sum_{q0 <= i < q1} w[b][i] * P[b][h][i][j] * max(0, dP[b][h][i][j])   for j < T
 * with P, w, q0, q1 as in gvk_attention_colsum_bf16; P and dP stay fp32.  Deterministic (no atomics).
 * gvk_relevance_step: r_out[b][j] = r_in[b][j] + (1 / H) * sum_h out[b][h][j]   (heads summed in order; r_out may alias r_in). */
int gvk_attention_gradcolsum_bf16(const void* qkv, const float* lse, const void* dctx, int ld_dctx, const float* w, int ld_w, float* out, int B,
                                  int T, int H, int ld_qkv, int q0, int q1, void* stream);
int gvk_relevance_step(const float* r_in, const float* colsum, float* r_out, int B, int T, int H, void* stream);
/* input gradients for explanations (csrc/input_grad.hip).  The patch embedding is a Conv3d with stride == kernel, so its input gradient is
 * the im2col gradient dcols f32 [B*nsum*N][pd*ph*pw] (row b*N + n = patch n of sample b in grid order, column (kd*ph + kh)*pw + kw, the
 * layout of gvk_patchify_*) put back in place:
 *   out[b] = beta * out[b] + sum_{j < nsum} alpha * V(b*nsum + j) * (x[b] - x0[b])      out, x, x0 f32 [B][1][D][H][W]
 * V(s) = the volume of dcols sample s; x == NULL drops the factor, x0 == NULL reads as 0; beta == 0 never reads out.  The sum over j is one
 * FMA per step in order (splitting it over calls with beta = 1 gives the same bits).  pw % 4 == 0, pointers 16-byte aligned.
 * gvk_patch_reduce_f32: out f32 [B][D/pd][H/ph][W/pw] = per-patch sum of |vol| (absval) or of vol; deterministic.
 * gvk_evp_highpass_sign / _linear: the backward of gvk_evp_highpass (out = |hp . X| on the slices depth_mask marks, |X| on the others).
 *   _sign:   out = dout o sign(hp . img)  (marked slices),  dout o sign(img)  (others)     (sign(0) = 0)
 *   _linear: out (+)= op . x  (marked slices),  x  (others)   -- with op = hp^T the adjoint of the linear part.  out must not alias x. */
int gvk_unpatchify_f32(const float* dcols, float* out, const float* x, const float* x0, int B, int D, int H, int W, int pd, int ph, int pw,
                       int nsum, float alpha, float beta, void* stream);
int gvk_patch_reduce_f32(const float* vol, float* out, int B, int D, int H, int W, int pd, int ph, int pw, int absval, void* stream);
int gvk_evp_highpass_sign(const float* img, const float* hp, const int32_t* depth_mask, const float* dout, float* out, int B, int D, int H, int W,
                          void* stream);
int gvk_evp_highpass_linear(const float* x, const float* op, const int32_t* depth_mask, float* out, int accumulate, int B, int D, int H, int W,
                            void* stream);

/* ------------------------------------------------------------------ rank-L ("skinny") fp32 projections of the trainable
 * side paths, L in {4, 8, 16, 20, 32}.  GAViKO: gaviko.py:231-232,242 (MWSA norm/proj_down/qkv/proj_up) and
 * gaviko.py:155-156,187 (GPA proj_down+QuickGELU / proj_up), plus their autograd dgrad / wgrad.
 *
 * down:  y[m][0:L] = act( LN?(drop?(x[m][:])) . W^T + bias );  optional  y2[m][0:L2] = y . W2^T
 *        act: 0 none, 1 QuickGELU (x*sigmoid(1.702x)); w_layout 0: W [L][C], 1: W [C][L];
 *        ln_gamma/ln_beta non-NULL: LayerNorm(eps) of the row first (mean/rstd saved when non-NULL);
 *        drop_p > 0: the input row is multiplied by the counter-based dropout mask(seed, m*C + c) / (1-p). */
typedef struct gvk_skinny_down_desc {
  const float* x; const float* w; const float* bias;
  const float* ln_gamma; const float* ln_beta; float* mean; float* rstd;
  float* z; float* y;               /* pre-activation / activated output [M][L], either may be NULL */
  const float* w2; float* y2;       /* second stage, W2 [L2][L] */
  const uint64_t* seed_ptr;          /* optional device word added to `seed` at run time (HIP-graph-safe dropout) */
  int32_t M, C, L, L2, act, w_layout;
  int32_t act_in;                    /* 1: QuickGELU applied to the input rows before the projection (DVPT share_MLP, dvpt.py:38) */
  float eps, drop_p;
  uint64_t seed;
} gvk_skinny_down_desc;
int gvk_skinny_down(const gvk_skinny_down_desc* d, void* stream);

/* up:    v = drop?( lat[m][0:L] . W^T + bias );  out = accumulate ? out + v : (res ? res + v : v)
 *        w_layout 0: W [C][L], 1: W [L][C].  lat_override (optional, [B][P][L]): rows with (m % T) < P take their latent
 *        from lat_override[(m / T) * P + m % T] (GPA: prompt rows replaced by the fused context, gaviko.py:181-185). */
typedef struct gvk_skinny_up_desc {
  const float* lat; const float* w; const float* bias; const float* res; float* out; const float* lat_override;
  const uint64_t* seed_ptr;
  /* optional LayerNorm-backward epilogue: out = base + LN'(v) with v = lat . W^T as the LN output gradient (no bias/dropout) */
  const float* ln_x; const float* ln_mean; const float* ln_rstd; const float* ln_gamma;
  void* out_bf16;                   /* optional bf16 copy of out (plain epilogue only) */
  const float* alpha_ptr;           /* optional device scalar: v = alpha * (lat . W^T + bias)          (DVPT prompt_gate, dvpt.py:46) */
  const float* gg_x;                /* optional f32 [M][C]: v *= QuickGELU'(gg_x[m][c])                 (dgrad through DVPT's input GELU) */
  /* optional second projection of the rows just written (plain epilogue only): z2 = out[m] . W2^T + bias2, y2 = act2(z2); W2 [L2][C]
     (GPA's proj_down of the new local tokens, gaviko.py:156, rides on the MWSA up-projection that produces them, gaviko.py:242) */
  const float* w2; const float* bias2; float* z2; float* y2;
  /* optional, with the LayerNorm-backward epilogue, w_layout 1 and w2 (L = 20 tile kernels only): a second rank-L term behind it,
     out = base + LN'(lat . W^T) + lat_b . W_b^T (W_b [L][C]), and the second projection reads `out` through the dropout mask (drop2_p, seed2):
     z2 = (out o mask) . W2^T with W2 in w2_layout (0: [L2][C], 1: [C][L2]).  One pass for three steps of the MWSA backward across a layer
     boundary: dL_in = dL_out + LN'(dlat . Wd) of layer i+1 (gaviko.py:231), dL += dzl . Wd_gpa of layer i (:156), dctx = proj_drop'(dL) . Wup
     of layer i (:242-243) */
  const float* lat_b; const float* w_b;
  /* optional, plain epilogue (L = 20 tile kernels only): the NEXT layer's MWSA entry on the rows just written (gaviko.py:231-232 of layer
     i+1 behind :242 of layer i), so the local stream is read once per layer instead of twice:
     nx_lat = LayerNorm(out; nx_ln_gamma, nx_ln_beta, nx_eps) . nx_w^T + nx_bias (nx_w [L][C]; nx_mean / nx_rstd [M] saved),
     nx_y2 = nx_lat . nx_w2^T (nx_w2 [nx_L2][L], nx_L2 <= 64: the qkv projection) */
  const float* nx_w; const float* nx_bias; const float* nx_ln_gamma; const float* nx_ln_beta; float* nx_mean; float* nx_rstd; float* nx_lat;
  const float* nx_w2; float* nx_y2;
  int32_t M, C, L, T, P, w_layout, accumulate;
  int32_t L2, act2, w2_layout, nx_L2;
  float drop_p, drop2_p, nx_eps;
  uint64_t seed, seed2;
} gvk_skinny_up_desc;
int gvk_skinny_up(const gvk_skinny_up_desc* d, void* stream);
/* out f32 [B*T][C] rows b*T + p (p < P) += (enh[b][p] - lat[b*T + p]) . w^T, w f32 [C][L]: the prompt rows of the GPA up-projection
 * (gaviko.py:183-187) when the plain-latent part rides the MLP GEMM as K-concatenation (gvk_pack_split_bf16) */
int gvk_prompt_up_fix(const float* enh, const float* lat, const float* w, float* out, int B, int T, int P, int C, int L, void* stream);
/* The same for a layer whose FIRST LayerNorm is folded into its qkv projection (gvk_gemm_desc.ln_mean): besides fixing the P prompt rows of
 * out (and of its bf16 copy out16, the folded GEMM's A operand) it finishes the row statistics -- mean / rstd f32 [B*T] of every row, from
 * the per-row partials part f32 [nparts][B*T][2] the fc2 GEMM left (gvk_gemm_desc.stat_part: sums of (x - pivot[m]) and of its square;
 * pivot f32 [B*T] = that GEMM's stat_pivot, NULL = 0), of the prompt rows from the rows themselves (two-pass). */
int gvk_prompt_up_fix_stats(const float* enh, const float* lat, const float* w, float* out, void* out16, const float* part, int nparts,
                            const float* pivot, float* mean, float* rstd, int B, int T, int P, int C, int L, float eps, void* stream);

/* outer: out[l][c] (transposed=0) or out[c][l] (transposed=1) (+)= sum_m narrow[m][l] * wide'[m][c];
 *        colsum[c] (+)= sum_m wide'[m][c] (optional).  wide' = LN(wide) when mean/rstd(/gamma/beta) are given, times the
 *        dropout mask when drop_p > 0.  scratch: f32 [128*(L+1)*C]; M (+ M2) <= 10240.  Deterministic (two-stage, no atomics). */
typedef struct gvk_outer_desc {
  const float* narrow; const float* wide; const float* lat_override;
  const float* mean; const float* rstd; const float* ln_gamma; const float* ln_beta;
  float* scratch; float* out; float* colsum;
  const uint64_t* seed_ptr;
  const float* narrow2; const float* wide2; /* optional second source [M2][L] / [M2][C] summed into the same result in the same pass
                                               (one weight fed by two token streams: GPA proj_down, gaviko.py:155-156); plain rows only */
  int32_t M, C, L, T, P, transposed, accumulate;
  int32_t wide_act;                  /* 1: QuickGELU applied to `wide` on the fly (DVPT: dW_d = dz^T . QuickGELU(x)) */
  int32_t M2;
  float drop_p;
  uint64_t seed;
} gvk_outer_desc;
int gvk_outer_reduce(const gvk_outer_desc* d, void* stream);
/* Gradients of y = LN(x) . W^T (W [L][C]) from Q[l][c] = sum_m dy[m][l] xhat[m][c] (gvk_outer_reduce with mean/rstd but no gamma/beta)
 * and S[l] = sum_m dy[m][l]:  dW (+)= gamma*Q + beta (x) S,  dgamma (+)= sum_l W*Q,  dbeta (+)= sum_l W*S,  dbias (+)= S (may be NULL). */
int gvk_ln_lowrank_affine(const float* Q, const float* S, const float* W, const float* gamma, const float* beta, float* dW, float* dgamma,
                          float* dbeta, float* dbias, int L, int C, int accumulate, void* stream);
/* out[j][l] (+)= sum_m a[m][j] * b[m][l]  (J, L <= 64); scratch f32 [64*J*L] */
int gvk_small_wgrad(const float* a, const float* b, float* out, float* scratch, int M, int J, int L, int accumulate, void* stream);
/* Several small reductions batched into one pair of launches (deterministic, two stages).  b == NULL: out[j] (+)= sum_m a[m][j],
 * j < J.  b != NULL: out[j][l] (+)= sum_m a[m][j] * b[m][l].  Up to 8 jobs per call; jobs of one call must not share `out`.
 * scratch: f32 [32 * total number of outputs]. */
typedef struct gvk_reduce_job {
  const float* a; const float* b; float* out;
  const float* a2;                   /* column sums only (b == NULL): M2 more rows [M2][J] summed into the same outputs */
  int32_t M, J, L, accumulate, M2;
} gvk_reduce_job;
int gvk_reduce_batch(const gvk_reduce_job* jobs, int njobs, float* scratch, void* stream);
/* Every parameter gradient of one rank-L side-path module of one layer in ONE launch (csrc/paramgrad.hip): up to 3 outer products
 *   out[l][c] (transposed=0) or out[c][l] (transposed=1) (+)= sum_m narrow'[m][l] * wide'[m][c],   colsum[c] (+)= sum_m wide'[m][c]
 * (narrow f32 [M][L], wide f32 [M][C]; narrow' = narrow with the rows t < P of every T-row sample taken from lat_override [.][P][L];
 * wide' = (wide * the dropout mask of element (m, c) when drop_p > 0, - mean[m]) * rstd[m] when mean / rstd are given -- the mask first,
 * as in gvk_outer_reduce; a second
 * source (narrow2, wide2, M2 plain rows) extends the same sum -- one weight fed by two token streams, gaviko.py:155-156), and up to 8
 * small reductions (gvk_reduce_job) over the same rows.  With aff_w (f32 [L][C] = the projection weight behind a LayerNorm, wide' = xhat)
 * the product Q is not stored: out[l][c] (+)= gamma_c Q[l][c] + beta_c S[l], aff_dgamma[c] (+)= sum_l w[l][c] Q[l][c],
 * aff_dbeta[c] (+)= sum_l w[l][c] S[l], aff_dbias[l] (+)= S[l] with S[l] = sum_m narrow[m][l] (gaviko.py:231: autograd of LN + proj_down).
 * Deterministic: partial tiles are summed in slab order by the workgroup that arrives last at a column tile's ticket word; no atomics on
 * data.  The hand-off issues NO release fence: partials leave as write-through (sc1) stores, every storing wave drains them
 * (s_waitcnt vmcnt(0)) before the workgroup barrier behind which one lane takes the agent-scope ticket, and only the last arriver runs
 * an agent-scope ACQUIRE (drops its CU's stale L1 lines) before reading -- the write-through form of the MI355X guide's hand-off recipe;
 * the ordering rests on sc1 stores having left the XCD once vmcnt retires them, not on a language-level release.  scratch f32 [gvk_param_grads_scratch(...)], tickets int32 [n_tickets] ZERO at allocation (the
 * kernel leaves them zero); calls that share scratch / tickets must be ordered by their stream.  C % 4 == 0, L % 4 == 0, L <= 28. */
typedef struct gvk_pgrad_outer {
  const float* narrow; const float* wide; const float* narrow2; const float* wide2; const float* lat_override;
  const float* mean; const float* rstd;
  float* out; float* colsum;
  const float* aff_w; const float* aff_gamma; const float* aff_beta; float* aff_dgamma; float* aff_dbeta; float* aff_dbias;
  int32_t M, M2, T, P, transposed, accumulate;
  int32_t C;                         /* columns (= row stride) of THIS job's wide operand; 0 = the call's C */
  float drop_p;
  uint64_t seed;
} gvk_pgrad_outer;
int64_t gvk_param_grads_scratch(const gvk_pgrad_outer* outer, int n_outer, const gvk_reduce_job* small, int n_small, int C, int L);
int gvk_param_grads(const gvk_pgrad_outer* outer, int n_outer, const gvk_reduce_job* small, int n_small, float* scratch,
                    int64_t scratch_elems, int32_t* tickets, int n_tickets, const void* seed_ptr, int C, int L, void* stream);
/* out[c] (+)= sum_m x[m][c]; scratch f32 [64*C] */
int gvk_colsum(const float* x, float* out, float* scratch, int M, int C, int accumulate, void* stream);

/* ------------------------------------------------------------------ GAViKO masked-window local self-attention core (fp32)
 * qkv f32 [B*N][3L] = [q | k | v] latents; single head; scale = model_dim^-0.5 (gaviko.py:201, NOT L^-0.5).
 * The 0/-inf [N,N] mask of gaviko.py:212-227 is index arithmetic here: query (d,h,w) attends key (d',h',w') iff
 * d - kd/2 <= d' < d - kd/2 + kd (likewise h, w), clipped to the DxHxW patch grid.  attn_drop (gaviko.py:239) is a
 * counter-based mask(seed, (b*N+i)*N + j) so that the backward regenerates it.
 * fwd writes ctx [B*N][L], lse [B*N];  bwd needs those + dctx and writes dqkv [B*N][3L] (delta [B*N] is scratch). */
typedef struct gvk_window_attn_desc {
  const float* qkv; float* ctx; float* lse;
  const float* dctx; float* delta; float* dqkv;
  const uint64_t* seed_ptr;
  int32_t B, D, H, W, kd, kh, kw, L;
  float scale, drop_p;
  uint64_t seed;
} gvk_window_attn_desc;
int gvk_window_attn_fwd(const gvk_window_attn_desc* d, void* stream);
int gvk_window_attn_bwd(const gvk_window_attn_desc* d, void* stream);

/* ------------------------------------------------------------------ GAViKO gated prompt awakening core (fp32), gaviko.py:159-185
 * Works on the activated latents xl [B*T][L] (global: rows [P prompts | cls | N image]) and ll [B*N][L] (local).
 * fwd: gates + both cross-attentions -> enh [B][P][L] (what replaces the prompt rows before proj_up); the other
 *      outputs are saved for the backward.  bwd: consumes dcomb [B*T][L] (= d proj_up input) and writes the gradients
 *      wrt the proj_down pre-activations (dzx [B*T][L], dzl [B*N][L]), dqg/dql [B][P][L] (query-projection outputs;
 *      wgrad = gvk_small_wgrad(dq, prm)), and gate_partials [B][gvk_gpa_gate_param_count(L,P)] -- per-sample gradients
 *      of [ca0_g L | ca0_b L | ca1_w 64L | ca1_b 64 | ca3_w 64P | ca3_b P | gl0_g L | gl0_b L | gl1_w L | gl1_b 1]
 *      (sum over B with gvk_colsum).  scale = L^-0.5 (gaviko.py:76). */
typedef struct gvk_gpa_desc {
  const float* xl; const float* ll;
  const float* ca0_g; const float* ca0_b; const float* ca1_w; const float* ca1_b; const float* ca3_w; const float* ca3_b;
  const float* gl0_g; const float* gl0_b; const float* gl1_w; const float* gl1_b;
  const float* wgq; const float* bgq; const float* wlq; const float* blq;
  float* imp; float* gw; float* enh;
  float* prm; float* qg; float* ql; float* cg; float* cl; float* lse_g; float* lse_l;
  const float* dcomb; const float* zx; const float* zl;
  float* dimp; float* dgw_part;
  float* dqg; float* dql; float* dcg; float* dcl; float* delta_g; float* delta_l; float* dprm;
  float* dcls; float* gate_partials; float* dzx; float* dzl;
  void* enh16;            /* optional (fwd): split-bf16 copy [hi | lo | hi] of enh[b][p][:] (gvk_pack_split_bf16, activation side) into row
                             b*T + p, columns col16 .. col16 + 3L - 1 of a [B*T][ld16] GEMM operand */
  int32_t B, T, N, P, L, ld16, col16;
  float scale;
} gvk_gpa_desc;
int gvk_gpa_fwd(const gvk_gpa_desc* d, void* stream);
int gvk_gpa_bwd(const gvk_gpa_desc* d, void* stream);
int gvk_gpa_gate_param_count(int L, int P);

/* ------------------------------------------------------------------ probability maps of the two GAViKO attentions for explanations
 * (csrc/gaviko_maps.hip).  Neither forward builds a probability; both maps are recomputed from what a forward leaves, against its own
 * log-sum-exp, as the backward passes do.  Deterministic (no atomics); launched on the given stream, not part of a launch plan.
 *
 * gvk_window_attn_colsum: weighted rows of the MWSA probability matrix (what a hook on F.softmax of gaviko.py:238 sees), never materialised:
 *   out f32 [B][N]  out[b][j] = sum_i w[b][i] * P[b][i][j],   P[b][i][j] = exp(scale * q_i . k_j - lse[b][i]) for j in window(i), else 0
 * qkv, lse, the grid, the window and scale as gvk_window_attn_fwd takes / leaves them; w f32 [B][N].  One wave per key j over the
 * REVERSE window (the key-side pass of gvk_window_attn_bwd with w_i in the place of dctx_i). */
typedef struct gvk_window_colsum_desc {
  const float* qkv; const float* lse; const float* w; float* out;
  int32_t B, D, H, W, kd, kh, kw, L;
  float scale;
} gvk_window_colsum_desc;
int gvk_window_attn_colsum(const gvk_window_colsum_desc* d, void* stream);
/* gvk_gpa_attn_maps: the two cross-attention probability blocks of one GPA layer (gaviko.py:90-91) and their gated fusion (:175-178),
 * from the buffers gvk_gpa_fwd saved -- qg / ql are its PRE-SCALED queries (scale * (Wq prompt + bq)), lse_g / lse_l natural-log:
 *   pg[b][p][n]    = exp(qg[b][p] . xl[b][P+1+n] - lse_g[b][p])  for n >= P+1, else 0   (the reference slices the image tokens twice,
 *                    gaviko.py:161,107: the global softmax runs over rows 2P+2 .. T-1 of xl, patch positions P+1 .. N-1)
 *   pl[b][p][n]    = exp(ql[b][p] . ll[b][n] - lse_l[b][p])
 *   fused[b][p][n] = imp[b][p] * (gw[b] * pg + (1 - gw[b]) * pl)     -- the coefficient with which position n enters enhanced prompt p
 * outputs f32 [B][P][N], each may be NULL (not all three).  T = P + 1 + N, N > P + 1, P <= 64. */
typedef struct gvk_gpa_maps_desc {
  const float* xl; const float* ll; const float* qg; const float* ql; const float* lse_g; const float* lse_l; const float* imp; const float* gw;
  float* pg; float* pl; float* fused;
  int32_t B, T, N, P, L;
} gvk_gpa_maps_desc;
int gvk_gpa_attn_maps(const gvk_gpa_maps_desc* d, void* stream);

/* ------------------------------------------------------------------ token assembly and the pooled head
 * rows_broadcast: out[b][row_off + r][:] = src[r][:] + add[r][:]  (cls_token + pos[0]; prompts + prompt_pos;
 *                 vision_transformer.py:154-156, gaviko.py:536-543, vpt.py:127-131).  out is [B*T][C].
 * rows_batch_sum: out[r][:] (+)= sum_b dg[b][row_off + r][:]; out2 (optional) receives the same (two parameters that
 *                 enter as a sum share a gradient: prompt_embeddings / prompt_positional_embedding). */
int gvk_rows_broadcast(float* out, const float* src, const float* add, int B, int T, int row_off, int R, int C, void* stream);
int gvk_rows_batch_sum(const float* dg, float* out, float* out2, int B, int T, int row_off, int R, int C, int accumulate, void* stream);
/* head: logits[b] = Wh . mean_{r in [r0, r0+R)} LN(g[b][r]) + bh   -- the final LayerNorm is evaluated only on the rows
 * the head consumes (gaviko.py:306,316: rows 0..P; vision_transformer.py:89,161: row 0, or all rows for pool='mean').
 * bwd: dwh/dbh (+)= ...; dg rows r0..r0+R of every sample receive the LN backward (caller zero-fills the rest). */
typedef struct gvk_head_desc {
  const float* g; const float* ln_gamma; const float* ln_beta; const float* wh; const float* bh;
  float* logits; float* pooled;
  const float* dlogits; float* dg; float* dwh; float* dbh;
  int32_t B, T, C, K, r0, R, accumulate;
} gvk_head_desc;
int gvk_head_fwd(const gvk_head_desc* d, void* stream);
int gvk_head_bwd(const gvk_head_desc* d, void* stream);

/* ------------------------------------------------------------------ VPT (model/vpt.py)
 * small_linear: out[r][:] = W . x[r] + b for a handful of rows (prompt_proj = Linear(prompt_dim, C), vpt.py:56,127-131);
 *   bwd: dw[c][k] (+)= sum_r dout[r][c] x[r][k], db (+)= colsum(dout), dx[r][k] (+)= sum_c dout[r][c] w[c][k] (any output may be NULL).
 * vpt_repack: the per-layer sequence rebuild of deep VPT (vpt.py:147-153): out = [in[:,0] | prompt (P rows) | in[:, 1+skip:]],
 *   Tout = Tin - skip + P, skip = prompt_dim for layers > 0 (reference quirk: drops the old prompts AND skip-P patch tokens);
 *   bwd scatters dout back (rows 1..skip of din are zero).  Prompt-row gradients: gvk_rows_batch_sum. */
int gvk_small_linear_fwd(const float* x, const float* w, const float* b, float* out, int R, int K, int C, void* stream);
int gvk_small_linear_bwd(const float* x, const float* w, const float* dout, float* dw, float* db, float* dx, int R, int K, int C,
                         int accumulate, void* stream);
int gvk_vpt_repack_fwd(const float* in, const float* prompt, float* out, int B, int Tin, int Tout, int P, int skip, int C, void* stream);
int gvk_vpt_repack_bwd(const float* dout, float* din, int B, int Tin, int Tout, int P, int skip, int C, void* stream);
/* LoRA merge (model/melo.py:41-47): out f32 [3C][C] = W + s * [B_q.A_q ; 0 ; B_v.A_v], s = alpha // r, A [r][C], B [C][r].
 * The merged matrix is then cast to the bf16 GEMM operand (and its transpose for the dgrad) like any other weight. */
int gvk_lora_merge_f32(const float* w, const float* a_q, const float* b_q, const float* a_v, const float* b_v, float* out, int C, int r,
                       float s, void* stream);
/* bf16 [M][ld_in] column block -> dense f32 [M][C] (gradient blocks handed to the fp32 rank-r kernels) */
int gvk_cast_bf16_f32_strided(const void* in, float* out, int M, int C, int ld_in, void* stream);

/* ------------------------------------------------------------------ SSF, `--method ssf` (model/ssf.py)
 * ssf_ada(x, s, t) = x*s + t (ssf.py:24-31) always follows a LayerNorm or a Linear, so the forward runs the plain ViT
 * kernels on effective parameters and the backward adds two column sums per site.
 * gvk_ssf_fold_weight: out[n][k] = w[n][k]*s[n] (bf16, or fp32 when out_f32), out_t (may be NULL) = its transpose [K][N].
 * gvk_ssf_fold_vec:    out = a*s + t   (a NULL -> t alone: the bias-free to_qkv; t NULL -> a*s: a LayerNorm gamma).
 * gvk_ssf_colgrad:     dt[n] = sum_m dy[m][n];  ds[n] = sum_m dy[m][n]*z[m][n] with z = (y - t)/s the pre-ssf value,
 *                      y = y0 (bf16 / fp32) [- y1 fp32] [- pos[m % rows_in][n]]; optional row mapping as GVK_EPI_PATCH_F32;
 *                      scratch f32 [64*2*N].
 * gvk_ssf_ln_grad:     LayerNorm+ssf site, from the effective-affine gradients (gvk_layernorm_bwd_affine):
 *                      ds = gamma*dgamma' + beta*dbeta', dt = dbeta'.
 * gvk_ssf_head_grad:   the final norm + ssf in front of the head (only the pooled rows r0..r0+R carry gradient). */
typedef struct gvk_ssf_colgrad_desc {
  const void* dy; const void* y0; const float* y1; const float* pos;
  const float* s; const float* t; float* ds; float* dt; float* scratch;
  int32_t M, N, ld_dy, ld_y, dy_f32, y0_f32, rows_in, rows_out, row_off;
  int32_t y0_cols;   /* columns n < y0_cols of y0 are multiplied by y0_mul when read: undoes the attention pre-scale of the q block of a saved */
  float y0_mul;      /* qkv (gvk_gemm_desc.scale_cols), y0_mul = 1 / col_scale; 0 columns = off */
  float y_mul;       /* y = y_mul * (y0 - y1) - pos: a site whose output went through nn.Dropout before it was stored (to_out / fc2 + ssf_2 of an
                        unfrozen backbone, the patch embedding under emb_dropout) is read back as kept / (1 - p), so y_mul = 1 - p with dy = the
                        MASKED gradient (dropped elements then contribute nothing); 0 is taken as 1 */
} gvk_ssf_colgrad_desc;
int gvk_ssf_fold_weight(const float* w, const float* s, void* out, void* out_t, int N, int K, int out_f32, void* stream);
int gvk_ssf_fold_vec(const float* a, const float* s, const float* t, float* out, int n, void* stream);
int gvk_ssf_colgrad(const gvk_ssf_colgrad_desc* d, void* stream);
int gvk_ssf_ln_grad(const float* dgamma_eff, const float* dbeta_eff, const float* gamma, const float* beta, float* ds, float* dt, int n,
                    void* stream);
int gvk_ssf_head_grad(const float* g, const float* mean, const float* rstd, const float* wh, const float* dlogits, const float* gamma,
                      const float* beta, float* ds, float* dt, int B, int T, int C, int K, int r0, int R, void* stream);

/* ------------------------------------------------------------------ DVPT, `--method dvpt` (model/dvpt.py)
 * Latent-space core of share_MLP (dvpt.py:37-47) on z = proj_d(QuickGELU(x)) f32 [B*T][L] (gvk_skinny_down with act_in = 1;
 * rows per sample: P prompts | cls | T-P-1 patches):
 *   gvk_dvpt_fwd: enh[b][p] = softmax(scale * z_p . z_patches^T) . z_patches, lse saved            (scale = d_model^-1/2)
 *   gvk_dvpt_bwd: from dcomb = dy . W_u (NOT yet scaled by the gate) and colsum_dy = sum_m dy:
 *                 dgate = <dcomb, lat'> + <bu, colsum_dy>;  dz (all rows) = backward of the attention and of the concatenation
 * (the up-projection and the gate are gvk_skinny_up with lat_override / alpha_ptr; gvk_scale_dev applies the gate to dW_u, db_u). */
typedef struct gvk_dvpt_desc {
  const float* z; float* enh; float* lse;               /* z [B*T][L]; enh [B][P][L], lse [B][P]: written by fwd, read by bwd */
  const float* dcomb; const float* gate; const float* bu; const float* colsum_dy;
  float* delta; float* dz; float* dgate;                 /* delta [B][P] scratch; dz [B*T][L]; dgate [1] */
  int32_t B, T, P, L, C;
  float scale;
} gvk_dvpt_desc;
int gvk_dvpt_fwd(const gvk_dvpt_desc* d, void* stream);
int gvk_dvpt_bwd(const gvk_dvpt_desc* d, void* stream);
int gvk_scale_dev(float* x, const float* alpha, int64_t n, void* stream);   /* x[i] *= alpha[0], alpha on the device */

/* ------------------------------------------------------------------ EVP, `--method evp` (model/evp.py)
 * gvk_evp_highpass: PromptGenerator.fft (evp.py:126-147) as it executes on [B,1,D,H,W]: out[b,d] = |hp . img[b,d]| on the depth slices
 *   with depth_mask[d] != 0, |img[b,d]| on the others; hp f32 [H][H] = I - Re(F^-1 diag(band) F) and the slice mask are built by
 *   the host (gaviko_amd/engine.py::evp_highpass_operator) from the reference's mask indexing.  No FFT library involved.
 * The remaining entry points are glue for the rank-(dim/32) prompt latents (zero-padded to a width the rank-L kernels support):
 *   gvk_pad2d_f32   dst (drows x dcols) = src (rows x cols, optionally transposed), zero elsewhere
 *   gvk_add2d_f32   out = a + b on a rows x cols window with independent leading dimensions
 *   gvk_gelu_fwd/bwd_f32  exact (erf) GELU of the light-weight MLPs (evp.py:45-49) and dy * GELU'(x)
 *   gvk_rows_patch  tok[b][row_off+n] (= or +=) src[b*N+n] (+ pos[n])     (tokens = conv + pos; x[:,1:] += prompt_i, evp.py:235-238)
 *   gvk_rows_gather the inverse read (the prompt gradient is the patch rows of the layer-input gradient) */
int gvk_evp_highpass(const float* img, const float* hp, const int32_t* depth_mask, float* out, int B, int D, int H, int W, void* stream);
int gvk_pad2d_f32(const float* src, int ld_src, int rows, int cols, int transpose, float* dst, int ld_dst, int drows, int dcols, void* stream);
int gvk_add2d_f32(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int cols, void* stream);
int gvk_gelu_fwd_f32(const float* x, float* y, int64_t n, void* stream);
int gvk_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int gvk_rows_patch(float* tok, const float* src, const float* pos, int B, int T, int N, int C, int row_off, int accumulate, void* stream);
int gvk_rows_gather(const float* tok, float* dst, int B, int T, int N, int C, int row_off, void* stream);

/* ------------------------------------------------------------------ optimisation step
 * Replaces train.py:315-319: torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step() over every
 * trainable tensor, on the engine's flat fp32 gradient buffer (exp_avg / exp_avg_sq share its layout).
 * gvk_sumsq: out[0] = sum x^2, two-stage deterministic; scratch f32 [256].
 * gvk_adam_step: one workgroup per table row; blk_tab int32 [nblocks][4] = {tensor id, offset inside that tensor, offset
 * into the flat buffers, element count (<= 1024)}; ptr_tab uint64 [ntensors] = parameter data pointers.  norm_sq (device
 * scalar from gvk_sumsq over the same flat gradient) enables clipping: g *= min(1, max_norm / (sqrt(norm_sq) + 1e-6)),
 * written back as torch does.  lr / beta1 are the OneCycleLR values of this step (train.py:197-206, host-side schedule);
 * bias_c1 = 1 - beta1_product ... exactly torch's single-tensor Adam: p -= lr/bias_c1 * m / (sqrt(v)/sqrt(bias_c2) + eps). */
typedef struct gvk_adam_desc {
  const void* ptr_tab; const void* blk_tab;
  float* grad; float* m; float* v;
  const float* norm_sq;                    /* NULL: no clipping */
  int32_t nblocks;
  float lr, beta1, beta2, eps, bias_c1, bias_c2, max_norm;
} gvk_adam_desc;
int gvk_sumsq(const float* x, int64_t n, float* scratch, float* out, void* stream);
int gvk_adam_step(const gvk_adam_desc* d, void* stream);

/* ---- loss seed (caller side of the path) --------------------------------------------------------------------------
 * Replaces train.py:176-179 + 283/306 (criterion = FocalLoss(gamma=1.2) | CrossEntropyLoss; loss = criterion(outputs,
 * labels); loss.backward() seed) and the two per-step host reads of train.py:327-328.  One launch: loss[0] = the reduced
 * loss, dlogits = d loss / d logits, and (meter != NULL) meter[0] += loss*B, meter[1] += #(argmax == target),
 * meter[2] += B.  GVK_LOSS_FOCAL follows losses/focal_loss.py:84-115 as it executes (clamp to [eps, 1-eps] + softmax,
 * TWICE; weights = per-class rescaling or NULL; ignore_index rows contribute nothing).  target is int64 [B]. */
enum { GVK_LOSS_CE = 0, GVK_LOSS_FOCAL = 1 };
typedef struct gvk_loss_desc {
  const float* logits; const void* target; const float* weights;
  float* loss; float* dlogits; float* meter;
  int32_t B, K, kind, reduction;           /* reduction 0 = 'mean', 1 = 'sum', 2 = 'none' (loss then receives the B per-sample values, dlogits each row's own gradient) */
  float gamma, eps;
  int64_t ignore_index;
} gvk_loss_desc;
int gvk_loss_fwd_bwd(const gvk_loss_desc* d, void* stream);

/* ---- mixed targets and label smoothing (csrc/loss.hip, csrc/batchmix.hip): Mixup / CutMix across the data / loss boundary ----------
 * gvk_loss_mixed_fwd_bwd: the loss seed above for rows that carry TWO classes and a weight between them (timm's Mixup + SoftTargetCrossEntropy,
 *   kept as the pair it came from).  target_a, target_b int64 [B], lam float32 [B]; target_b and lam may both be NULL = no partner, lam = 1.
 *   l_i = lam_i l(x_i, a_i) + (1 - lam_i) l(x_i, b_i), 1 - lam_i formed in float32, l(x, t) the per-sample loss of gvk_loss_fwd_bwd with its class
 *   weight: GVK_LOSS_FOCAL as it executes (smoothing must be 0); GVK_LOSS_CE with smoothing e in [0, 1],
 *   l(x, t) = (1 - e) w_t (-log p_t) + (e / K) sum_k w_k (-log p_k), torch's label_smoothing rule for class-index targets.
 *   reduction 1 adds the l_i, 2 writes them, 0 divides their sum by sum_i (lam_i w_{a_i} + (1 - lam_i) w_{b_i}) over the rows that are not ignored
 *   (the weighted-mean rule of gvk_loss_fwd_bwd, which lam = 1 reproduces).  A row is ignored when a_i or b_i equals ignore_index: loss 0,
 *   gradient row 0.  dlogits = the gradient of the reduced loss (reduction 2: each row's own).  meter[0] and meter[2] as in gvk_loss_fwd_bwd;
 *   meter[1] += #(argmax == the dominant label: a_i when lam_i >= 0.5, else b_i).  A side whose coefficient is zero is not evaluated and both
 *   kernels call the same row functions, so smoothing = 0 with lam = 1 (or NULL) returns loss and dlogits bit for bit as gvk_loss_fwd_bwd does.
 *   One workgroup, one thread per row, strided over B.
 * gvk_batch_mix: the data side, one streaming pass for a batch in which every sample drew its own mode; x, out float32 [B][D][H][W], out must
 *   not overlap x; mode, perm int32 [B], lam float32 [B], box int32 [B][6] are DEVICE tables.  With p = perm[b]:
 *   GVK_MIX_COPY: out[b] = x[b] bit for bit; lam, perm and box are not read for that sample.
 *   GVK_MIX_MIXUP: out[b] = lam[b] * x[b] + (1 - lam[b]) * x[p] in float32, 1 - lam[b] formed in float32 in the kernel, in the TWO-ROUNDING form
 *     (each product rounded, then the sum: nothing is contracted), except that a term whose coefficient is exactly 0 is left out and not
 *     read: lam = 1 gives x[b] and lam = 0 gives x[p], bit for bit.
 *   GVK_MIX_CUTMIX: box[b] = (d0, d1, h0, h1, w0, w1), half-open: out[b] = x[p] inside the box and x[b] outside, bit for bit; lam is not read.
 *     An empty box gives x[b], a full box x[p].
 *   The kernel trusts perm in [0, B) and boxes inside the volume (the caller checks its host tables before the upload).  No atomics; copy
 *   and CutMix read one source voxel per output voxel, Mixup two.  16-byte accesses for a sample whose addresses are all on the 16-byte grid
 *   (sample b starts at x + b V: with V odd every second sample is off it and runs voxel by voxel), four scalar loads for a group of four that
 *   the box's edge or a row's end cuts, a scalar tail of V % 4 voxels.  B <= 65535, D*H*W < 2^31, no divisibility or alignment requirement. */
enum { GVK_MIX_COPY = 0, GVK_MIX_MIXUP = 1, GVK_MIX_CUTMIX = 2 };
typedef struct gvk_loss_mixed_desc {
  const float* logits; const void* target_a; const void* target_b; const float* lam; const float* weights;
  float* loss; float* dlogits; float* meter;
  int32_t B, K, kind, reduction;           /* as in gvk_loss_desc */
  float gamma, eps, smoothing;
  int64_t ignore_index;
} gvk_loss_mixed_desc;
int gvk_loss_mixed_fwd_bwd(const gvk_loss_mixed_desc* d, void* stream);
int gvk_batch_mix(const float* x, float* out, const int32_t* mode, const float* lam, const int32_t* perm, const int32_t* box, int B, int D, int H, int W,
                  void* stream);

/* ---- data side and evaluation metrics ------------------------------------------------------------------
 * Replace the torchio transforms of train.py:38-62 on a batch of raw volumes x [B][V] (V = D*H*W, float32, resident in HBM):
 * gvk_volume_minmax: partials [B][gvk_minmax_partials()] = per-slab (min, max) pairs of every volume.
 * gvk_rescale_intensity: tio.RescaleIntensity(out_min_max): y = ((x - min) / (max - min)) * (out_max - out_min) + out_min in
 *   float32, in that order; a constant volume passes through unchanged; minmax (optional) receives [B][2].  In place allowed.
 * gvk_spatial_transform: tio.RandomAffine + tio.RandomFlip as ONE resampling pass: out[b] at output voxel q reads in[b] at
 *   A_b . mirror(q) + t_b (mats [B][12], row-major 3x4 in array-axis order) with trilinear weights; neighbours outside the volume
 *   read the volume minimum (partials of the INPUT).  flags[b]: bits 0..2 = mirror axis 0..2, bit 3 = affine live (else exact gather).
 * Replace eval.py:103-122: gvk_eval_rows: proba = softmax(logits), pred = argmax, confusion uint64 [K][K] += (target, pred);
 * gvk_ovr_auc_counts: counts uint64 [K][3] += {2*#(p_pos > p_neg) + #(p_pos == p_neg), n_pos, n_neg} per class (one-vs-rest). */
int gvk_volume_minmax(const float* x, float* partials, int B, int64_t V, void* stream);
int gvk_minmax_partials(void);
int gvk_rescale_intensity(const float* x, const float* partials, float* y, float* minmax, int B, int64_t V, float out_min, float out_max, void* stream);
int gvk_spatial_transform(const float* in, float* out, const float* mats, const int32_t* flags, const float* partials, int B, int D, int H, int W,
                          void* stream);
int gvk_eval_rows(const float* logits, const void* target, float* proba, int32_t* pred, void* confusion, int N, int K, void* stream);
int gvk_ovr_auc_counts(const float* proba, const void* target, void* counts, int N, int K, void* stream);

/* ---- intensity augmentation (csrc/intensity.hip): the intensity group of train.py:43-48 (RandomMotion: next section) ---------
 * Volumes are float32 [B][D][H][W], one channel, resident in HBM; every table below is a DEVICE array with one row per sample, so one
 * launch serves a batch in which each sample drew a different transform or none.  Parity with torchio itself is unpinned.
 * gvk_gaussian_blur3d: tio.RandomBlur = scipy.ndimage.gaussian_filter(x, sigma=(s0, s1, s2)) with scipy's defaults: mode='reflect' (any
 *   radius, also above the axis length), truncate = 4.0.  The HOST builds the taps: radius [B][3] = int(4 sigma + 0.5) (0 on an axis with
 *   sigma <= 1e-15, which scipy skips), weights [B][3][2 GVK_BLUR_MAX_RADIUS + 1] = exp(-0.5 k^2 / sigma^2) normalised to sum 1 in float64,
 *   rounded to float32, taps 0..2r of an axis at the start of its row (radius 0: the single weight 1).  max_radius states the largest entry
 *   of radius; above GVK_BLUR_MAX_RADIUS (sigma above 4) the call is rejected, and the kernels clamp what they read to that cap.  fp32
 *   accumulation.  Two passes over HBM: H and W together through LDS into scratch [B][D*H*W] (caller-provided), then D down coalesced
 *   columns into out.  in, out and scratch are three different buffers.  A sample with radius (0, 0, 0) comes back bit-identical.
 * gvk_intensity_pointwise: one streaming pass, y may be x.  kind [B]: 0 copy; 1 tio.RandomNoise, y = x + (std z(i) + mean) with noise
 *   [B][2] = (std, mean), seeds uint64 [B] and z(i) = sqrtf(-2 logf(u1)) cosf(2 pi u2), u1 = ((h(seed, 2i) >> 8) + 1) 2^-24,
 *   u2 = (h(seed, 2i+1) >> 8) 2^-24, h = the element hash of gvk_dropout_rows, i = voxel index inside the volume; 2 tio.RandomBiasField,
 *   y = x expf(P(c0, c1, c2)), ck = (k - (n_k - 1)/2) / ((n_k - 1)/2) along array axis k (0 when n_k = 1), P = sum of coeff[j] c0^a c1^b c2^c
 *   over a in 0..order, b in 0..order-a, c in 0..order-a-b nested in that order with j counting up; coeff [B][GVK_BIAS_COEFFS], order <= 3 for
 *   the whole launch.  All three tables must be valid pointers whatever the kinds.  16-byte aligned volumes, D*H*W a multiple of 4. */
enum { GVK_BLUR_MAX_RADIUS = 16, GVK_BIAS_COEFFS = 20 };
int gvk_gaussian_blur3d(const float* in, float* out, float* scratch, const float* weights, const int32_t* radius, int max_radius, int B, int D, int H,
                        int W, void* stream);
int gvk_intensity_pointwise(const float* x, float* y, const int32_t* kind, const float* noise, const void* seeds, const float* coeff, int order, int B,
                            int D, int H, int W, void* stream);

/* ---- tio.RandomMotion (csrc/motion.hip): the fourth member of that group, k-space motion ghosting, in one fused pass -------------
 * torchio composites the shifted 3-D spectra of the volume and of K rigidly moved copies in K+1 slabs along the LAST array axis.  The slab
 * masks do not depend on the other two frequency axes, so the transforms over D and H cancel and a real circular convolution along W is
 * left per image -- no FFT:  out[b][d][h][w] = sum_{s=0..K} sum_{w'} ctab[b][s][(w - w') mod W] * img_s[b][d][h][w'],
 * img_0 = in[b], img_k = in[b] resampled through mats[b][k-1] (row-major 3x4, output voxel -> input position, exactly the arithmetic and
 * pad rule of gvk_spatial_transform with the affine live: trilinear, neighbours outside read the volume minimum taken from partials =
 * gvk_volume_minmax of in).  ctab [B][K+1][W] is built on the host in float64 (data.motion_tables): row s = (1/W) sum over the
 * frequencies j of the slabs that image s fills of cos(2 pi (j - W/2) m / W), W/2 the integer quotient (W//2, also for odd W); the rows sum to the unit impulse.  The moved images never
 * reach HBM: a workgroup gathers 32 (d, h) lines of one image into LDS and multiplies them by the circulant of its ctab row on the f32-input
 * matrix cores (fp32 operands, fp32 accumulation, a fixed order: the same bits on every run), image after image into the same accumulators.
 * live [B]: a sample with live[b] == 0 is copied, bit for bit.  K in 1..GVK_MOTION_MAX_TRANSFORMS, W in 2..GVK_MOTION_MAX_W, in and out must
 * not overlap; no divisibility or alignment requirement on D, H, W. */
enum { GVK_MOTION_MAX_TRANSFORMS = 4, GVK_MOTION_MAX_W = 256 };
int gvk_motion_artifact(const float* in, float* out, const float* mats, const float* ctab, const int32_t* live, const float* partials, int K, int B,
                        int D, int H, int W, void* stream);

/* ---- tio.RandomElasticDeformation (csrc/elastic.hip): a cubic B-spline warp of the volume, in one pass ---------------------------
 * ITK's order-3 BSplineTransform over the image extent.  ctrl [B][n0][n1][n2][3]: control-point displacements in VOXELS, component a along
 * array axis a.  Per axis a with S voxels and n control points: M = n - 3 mesh cells of h = S / M voxels; output index q has
 * u = (q + 0.5) / h, i = min(floor(u), M - 1), t = u - i, and control points i..i+3 weigh B0 = (1-t)^3/6, B1 = (3t^3 - 6t^2 + 4)/6,
 * B2 = (-3t^3 + 3t^2 + 3t + 1)/6, B3 = t^3/6.  d(q) = the tensor product of the three axes' weights over the 4x4x4 control points (fp32,
 * contracted axis 1, then axis 0, then axis 2), and out[b] at q reads in[b] at float(q) + d(q) -- one fp32 add per axis -- with the
 * trilinear arithmetic and pad rule of gvk_spatial_transform: neighbours outside the volume read the volume minimum taken from partials =
 * gvk_volume_minmax of in.  field (may be NULL) receives [B][3][D][H][W] = exactly the d the read used.  live [B]: a sample with
 * live[b] == 0 is copied bit for bit and its field is zero.  4 <= n_a <= GVK_ELASTIC_MAX_CONTROL_POINTS (one grid size per launch); in, out
 * and field must not overlap; no divisibility or alignment requirement on D, H, W.  No atomics: the same bits on every run. */
enum { GVK_ELASTIC_MAX_CONTROL_POINTS = 16 };
int gvk_elastic_deform(const float* in, float* out, float* field, const float* ctrl, const int32_t* live, const float* partials, int B, int D, int H,
                       int W, int n0, int n1, int n2, void* stream);

/* ---- intensity normalisation (csrc/normalize.hip): tio.RescaleIntensity with percentiles and a mask, tio.ZNormalization ---------------
 * Volumes are float32 x [B][V], 1 <= V < 2^31, x (and y) 16-byte aligned; NO divisibility requirement on V (sample b starts at x + b V; heads
 * and tails are handled in the kernels).  Everything stays on the device: the three calls hand each other DEVICE tables and none reads the
 * host.  NaN input is out of scope.
 * gvk_volume_stats: stats [B][GVK_NORMALIZE_STATS] doubles = (min, max, mean of ALL voxels; the mask threshold t; n, mean and unbiased
 *   standard deviation of the MASKED voxels x > t; one unused word), count [B] int64 = n.  mask_mode 0: no mask (t = -inf, n = V);
 *   1: t = the mean of all voxels rounded to float32 (x > x.mean()); 2: t = threshold.  The standard deviation (want_std != 0, else 0) is
 *   sqrt(sum (x - mean)^2 / (n - 1)) with the deviations taken from that mean in a pass of their own; 0 when n < 2.  All sums are float64 in a
 *   fixed order (per thread ascending, a fixed tree over the workgroup, a fixed tree over at most GVK_NORMALIZE_SLABS slabs), no floating-point
 *   atomics: the same input gives the same bits on every run.  partials: scratch of B * GVK_NORMALIZE_SLABS * 4 doubles.
 * gvk_volume_order_stats: exact order statistics of the masked voxels (t and n read from stats) for Q <= GVK_NORMALIZE_MAX_PERCENTILES
 *   percentile fractions qj = percentile / 100 (computed by the caller; entries beyond Q are ignored).  Per sample and j: v = (double)(n - 1) * qj
 *   (one float64 multiply), i = floor(v), g = v - i, a = the i-th smallest masked value, b = the min(i + 1, n - 1)-th; pairs [B][Q][2] = (a, b);
 *   cutoffs [B][Q] = float32 of numpy's 'linear' rule on float64 operands, c = a + (b - a) g for g < 0.5, else b - (b - a) (1 - g), every operation
 *   rounded once (nothing contracted).  The selection is a most-significant-first radix select on an order-preserving 32-bit key (3 passes of
 *   11 / 11 / 10 bits) and is exact for every finite float32 input, denormals included; -0.0 and +0.0 are one value (a or b may come back with
 *   either sign bit).  Each pass counts the digit of the keys under the distinct prefixes the 2 Q ranks fall under: at most 8 prefixes,
 *   4 per sweep over the data (a 32 KB LDS histogram), so more than 4 cost a second sweep of that pass.  The histograms are merged with integer
 *   atomics, which are exact in any order.  An empty mask gives zeros.  workspace: B * GVK_NORMALIZE_ORDER_WS_WORDS uint32.
 * gvk_normalize_intensity: a finishing step writes params [B][8] doubles = (lo, hi, sub, div, mul, add, mean, std) and status [B] from stats
 *   (and cutoffs [B][Q], entries 0 and 1 = low and high), then ONE streaming pass writes y.
 *   GVK_NORMALIZE_RESCALE: torchio's rescale.  lo, hi = the cutoffs; in_min = clamp(min, lo, hi), in_max = clamp(max, lo, hi) (the extremes of
 *   the clipped volume); y = (((clip(x, lo, hi) - in_min) / in_range) * (out_max - out_min)) + out_min, four float32 steps with a true divide.
 *   GVK_NORMALIZE_ZNORM: y = float32(((double)x - mean) / std), mean and std those of the masked voxels.
 *   status: 0 normalised; 1 empty mask; 2 in_range == 0, or std == 0, or n < 2.  A sample with a non-zero status is copied bit for bit. */
enum { GVK_NORMALIZE_SLABS = 128, GVK_NORMALIZE_STATS = 8, GVK_NORMALIZE_MAX_PERCENTILES = 4, GVK_NORMALIZE_ORDER_WS_WORDS = 32 + 3 * 8 * 2048 };
enum { GVK_NORMALIZE_RESCALE = 1, GVK_NORMALIZE_ZNORM = 2 };
int gvk_volume_stats(const float* x, double* partials, double* stats, int64_t* count, int mask_mode, float threshold, int want_std, int B, int64_t V,
                     void* stream);
int gvk_volume_order_stats(const float* x, const double* stats, void* workspace, float* pairs, float* cutoffs, int Q, double q0, double q1, double q2,
                           double q3, int B, int64_t V, void* stream);
int gvk_normalize_intensity(const float* x, float* y, const double* stats, const float* cutoffs, int Q, double* params, int32_t* status, int mode,
                            float out_min, float out_max, int B, int64_t V, void* stream);

/* ---- histogram standardisation (csrc/normalize.hip): tio.HistogramStandardization (Nyul & Udupa) --------------------------------------
 * Same volumes, tables and preconditions as above; stats comes from gvk_volume_stats of the same x.  fractions_host and targets_host are
 * HOST arrays: they are copied into the kernels' arguments, never into device memory.  No host read, no floating-point atomics: the same
 * bits on every run.
 * gvk_volume_landmarks: gvk_volume_order_stats for 1 <= Q <= GVK_LANDMARKS_MAX percentile fractions fractions_host[Q] in one call: pairs
 *   [B][Q][2] and cutoffs [B][Q] equal its results bit for bit for the same fraction (same ranks, same keys, same cutoff arithmetic).  The
 *   radix select runs GVK_LANDMARKS_PASSES passes of 8-bit digits, every one of the 2 Q wanted ranks with a histogram slot of its own
 *   (32 slots x 256 bins = 32 KB of LDS), so a pass is exactly one sweep over the volume whatever Q, the data and the number of distinct
 *   prefixes are: 4 sweeps per call.  An empty mask gives zeros.  workspace: B * GVK_LANDMARKS_WS_WORDS uint32.
 * gvk_histogram_standardize: cutoffs [B][GVK_HISTSTD_KNOTS] are the volume's own landmarks k_j (float32, ascending), targets_host
 *   [GVK_HISTSTD_KNOTS] the trained ones m_j.  A one-thread-per-sample step writes params [B][GVK_HISTSTD_PARAMS] doubles = (k_0..k_10,
 *   slope_0..slope_9, icpt_0..icpt_9, one unused word) in float64, every operation rounded once: d_j = k_{j+1} - k_j, taken as +inf where
 *   d_j < epsilon; slope_j = (m_{j+1} - m_j) / d_j; icpt_j = m_j - slope_j k_j.  Then ONE streaming pass writes
 *   y = float32(slope_j (double)x + icpt_j), product and sum rounded once each (no FMA), j = the number of interior knots k_1..k_9 that
 *   are <= x (np.digitize, right = False; nine float32 compares): the first and last segment extrapolate.  The mask only chose the voxels
 *   the landmarks came from; every voxel is mapped.  status: 0 standardised; 1 empty mask -- such a sample is copied bit for bit. */
enum { GVK_LANDMARKS_MAX = 16, GVK_LANDMARKS_PASSES = 4, GVK_LANDMARKS_WS_WORDS = 128 + 4 * 32 * 256 };
enum { GVK_HISTSTD_KNOTS = 11, GVK_HISTSTD_PARAMS = 32 };
int gvk_volume_landmarks(const float* x, const double* stats, void* workspace, float* pairs, float* cutoffs, int Q, const double* fractions_host, int B,
                         int64_t V, void* stream);
int gvk_histogram_standardize(const float* x, float* y, const double* stats, const float* cutoffs, const double* targets_host, double epsilon,
                              double* params, int32_t* status, int B, int64_t V, void* stream);

/* ---- tio.RandomGhosting / RandomSpike / RandomGamma / RandomAnisotropy (csrc/kspace.hip): the rest of torchio's MRI augmentation family ----
 * Volumes are float32 [B][D][H][W], one channel, resident in HBM; every table is a DEVICE array with one row per sample and is never read by
 * the host, so one launch serves a batch in which each sample drew a different axis, a different transform or none.  A sample that drew
 * nothing (live[b] == 0, kind[b] == 0) is copied bit for bit, signed zeros and subnormals included.  in and out must not overlap; no
 * divisibility or alignment requirement on D, H, W; no atomics: the same bits on every run.  Parity with torchio itself is unpinned.
 * gvk_axis_circular_conv: ghosting.  Scaling planes of the shifted spectrum along ONE axis by a mask that does not depend on the other two
 *   frequency axes is a real circular convolution along that axis -- no FFT:  out[..i..] = sum_i' ctab[b][(i - i') mod N] * in[..i'..] along
 *   array axis axis[b] (0, 1, 2 = D, H, W; any other value is treated as live[b] == 0) of N voxels.  ctab [B][GVK_AXIS_CONV_MAX_N], entries
 *   0..N-1 of a row used, is built on the host in float64 (data.ghosting_tables): c[m] = delta[m] - (g / N) sum_{j in S} cos(2 pi (j - N/2) m / N),
 *   S = {0 <= j < N : j % n == 0, j != N/2}, N/2 the integer quotient.  The product runs on the f32-input matrix cores (fp32 operands, one
 *   rounding per product, fp32 accumulation in ascending i' = an fmaf chain).  Axis 2 multiplies 32 (d, h) lines by the circulant from the
 *   right (the product of gvk_motion_artifact with one image); axes 0 and 1 multiply a slab [N x 32 contiguous voxels] by it from the left, so
 *   global accesses run along W in all three forms; the circulant is read from a copy of the row in LDS and never exists in HBM; every output
 *   element is written once.  axis is not read by the host, so D, H and W must ALL be in 2..GVK_AXIS_CONV_MAX_N.
 * gvk_gamma_spike: one streaming pass.  kind [B]: GVK_KSPACE_COPY; GVK_KSPACE_GAMMA, y = copysignf(powf(|x|, gamma[b]), x) (zeros keep their
 *   sign; gamma[b] == 1 is the copy, exactly); GVK_KSPACE_SPIKE, nspikes[b] <= GVK_SPIKE_MAX spikes (clamped):
 *   y = x + scale * sum_s (c0 * (c1 * c2 - s1 * s2) - s0 * (s1 * c2 + c1 * s2)), every operation rounded once and nothing contracted, the sum
 *   in ascending s from 0.f, with (ca, sa) = tab[b][s][0 / 1][offset_a + x_a] = float32 of cos / sin(2 pi ((k_sa - N_a/2) x_a mod N_a) / N_a),
 *   tab [B][GVK_SPIKE_MAX][2][D + H + W] (offsets 0, D, D + H; data.spike_tables reduces the phase in integers and evaluates in float64), and
 *   scale = float32((double)amp[b] * |mean|), mean = column 2 of the stats row [B][GVK_NORMALIZE_STATS] of gvk_volume_stats of `in` (the
 *   float64 mean of all voxels): amp * |mean| is amp * max|F| / V for a non-negative volume.  Every table must be a valid pointer whatever
 *   the kinds.  D*H*W < 2^31.
 * gvk_axis_gather2: anisotropy.  Along array axis axis[b] of N voxels, with i the output index on that axis:
 *   out[..i..] = w[b][i] == 0 ? x0 : fmaf(w[b][i], x1 - x0, x0),  x0 = in[..src[b][i][0]..], x1 = in[..src[b][i][1]..];
 *   src int32 [B][n_max][2] (clamped to 0..N-1 on the device), w float32 [B][n_max], n_max >= max(D, H, W); data.anisotropy_tables does the
 *   coordinate arithmetic (nearest-neighbour downsampling, linear upsampling, edges clamped) in float64.  Lanes run along W for every axis. */
enum { GVK_AXIS_CONV_MAX_N = 256, GVK_SPIKE_MAX = 4 };
enum { GVK_KSPACE_COPY = 0, GVK_KSPACE_GAMMA = 1, GVK_KSPACE_SPIKE = 2 };
int gvk_axis_circular_conv(const float* in, float* out, const float* ctab, const int32_t* axis, const int32_t* live, int B, int D, int H, int W,
                           void* stream);
int gvk_gamma_spike(const float* in, float* out, const int32_t* kind, const float* gamma, const float* amp, const int32_t* nspikes, const float* tab,
                    const double* stats, int B, int D, int H, int W, void* stream);
int gvk_axis_gather2(const float* in, float* out, const int32_t* src, const float* w, const int32_t* axis, const int32_t* live, int n_max, int B, int D,
                     int H, int W, void* stream);

/* ---- nn.Dropout as its own pass (sites without a producing kernel to fuse into) ------------------------------------------
 * Replaces vision_transformer.py:157 (emb_dropout), vpt.py:129,148,152 (prompt_dropout) and carries the masks of the
 * Linear+Dropout pairs (vision_transformer.py:34,54) onto the gradient side.  out32 / out16 (either may be NULL, out32 may alias x)
 * = x * mask(seed + *seed_ptr, m*N + n) / (1 - drop_p) over logical rows m < M; with rows_in > 0 logical row m lives in buffer row
 * (m / rows_in) * rows_out + row_off + m % rows_in (a row range of every sample).  The mask function is the one of gvk_gemm_desc.drop_p. */
typedef struct gvk_dropout_desc {
  const float* x; float* out32; void* out16; const void* seed_ptr;
  int32_t M, N, ld, rows_in, rows_out, row_off;
  float drop_p;
  uint64_t seed;
} gvk_dropout_desc;
int gvk_dropout_rows(const gvk_dropout_desc* d, void* stream);

/* ---- perturbation of the input volume at patch granularity (csrc/perturb.hip): occlusion sensitivity, deletion / insertion curves ----
 * N = (D/pd)(H/ph)(W/pw) patches in patch-grid order, V = D*H*W voxels, S source volumes, Bout output samples of one chunk.  The per-output
 * tables (src, lo, hi, boxes, slot) are int32 DEVICE arrays: a sweep uploads them once and passes every chunk its slice.
 * gvk_patch_rank: rank i32 [S][N], rank[s][n] = #{m : rel[s][m] > rel[s][n]} + #{m < n : rel[s][m] == rel[s][n]} -- the inverse permutation of
 *   a stable descending argsort of rel f32 [S][N].  N <= 16384.  NaN is the caller's to reject.  Deterministic.
 * gvk_patch_mask_rank: mask u8 [Bout][N] = lo[o] <= rank[src[o]][n] < hi[o]            (deletion at k: (0, k); insertion at k: (k, N)).
 * gvk_patch_mask_box:  mask u8 [Bout][N] = patch n inside boxes[o] = {d0, d1, h0, h1, w0, w1} (half-open, patch-grid units, clipped by the grid).
 * gvk_perturb_volume:  out f32 [Bout][V], out[o][v] = mask[o][patch(v)] ? fill : x[src[o]][v] with fill = fill_scalar[src[o]] or
 *   base[nbase == 1 ? 0 : src[o]][v] (exactly one of the two pointers; nbase = 1 or S).  A selection of 32-bit words: bit-exact.  16-byte
 *   accesses when pw % 4 == 0 and the pointers are 16-byte aligned, one voxel per thread otherwise.  out must not overlap x.
 *   Bytes: Bout*V*4 written, at most (S + nbase)*V*4 read.
 * gvk_perturb_scores:  per output sample o with slot[o] in [0, nslots): prob[slot[o]] = softmax(logits[o])[target[src[o]]] (fp32, max-subtracted),
 *   logit[slot[o]] = logits[o][target[src[o]]], rows (optional) [nslots][K] row slot[o] = logits[o].  slot[o] < 0 writes nothing.  prob ==
 *   logit == NULL: the rows only (src / target unused).  Deterministic.
 * gvk_curve_auc:       auc[s] = trapezoid area of prob f32 [S][P] over x_i = ks[i] / N (ks int32 [P], device).  Deterministic. */
int gvk_patch_rank(const float* rel, int32_t* rank, int S, int N, void* stream);
int gvk_patch_mask_rank(const int32_t* rank, const int32_t* src, const int32_t* lo, const int32_t* hi, uint8_t* mask, int Bout, int S, int N,
                        void* stream);
int gvk_patch_mask_box(const int32_t* boxes, uint8_t* mask, int Bout, int nd, int nh, int nw, void* stream);
int gvk_perturb_volume(const float* x, const uint8_t* mask, const int32_t* src, const float* fill_scalar, const float* base, int nbase,
                       float* out, int Bout, int S, int D, int H, int W, int pd, int ph, int pw, void* stream);
int gvk_perturb_scores(const float* logits, const int32_t* src, const int32_t* target, const int32_t* slot, float* prob, float* logit,
                       float* rows, int Bout, int S, int K, int nslots, void* stream);
int gvk_curve_auc(const float* prob, const int32_t* ks, float* auc, int S, int P, int N, void* stream);

/* ---- predictive uncertainty and calibration (csrc/uncertainty.hip): Monte-Carlo dropout, flip test-time augmentation, reliability bins ----
 * gvk_tta_volumes: out f32 [Bout][D][H][W], out[o] = x[src[o]] mirrored along the axes named by the bits of flip[o] (bit 0 = D, bit 1 = H,
 *   bit 2 = W); flip[o] = 0 is a plain replica.  x f32 [S][D][H][W]; src / flip int32 [Bout] DEVICE tables (src within [0, S)).  A move of
 *   32-bit words: bit-exact.  16-byte accesses when W % 4 == 0 and the pointers are 16-byte aligned (the W mirror reads the mirrored float4
 *   and reverses its lanes), one voxel per thread otherwise.  out must not overlap x; Bout * D*H*W < 2^31.  Bytes: Bout*V*4 written, as many read.
 * gvk_predictive_stats: member_logits f32 [B][S][K] (B samples, S members each) -> per sample
 *     probs f32 [B][K]        mean over the members of softmax(logits) (max-subtracted, fp32)
 *     pred i32 [B]            argmax of probs, lowest index on an exact tie
 *     entropy [B]             H[mean p] in nats (0 log 0 = 0)
 *     expected_entropy [B]    mean over the members of H[p_s]
 *     mutual_info [B]         max(entropy - expected_entropy, 0)
 *     variation_ratio [B]     1 - max_k votes[k] / S
 *     std f32 [B][K]          population standard deviation of the member probabilities (two passes: exactly 0 for S = 1)
 *     votes i32 [B][K]        how many members have their own argmax (lowest index on a tie) at k
 *   One wave per sample, no atomics: deterministic.  S >= 1; 2 <= K <= 256 (4 classes per lane in registers).
 * gvk_calibration_bins: proba f32 [N][K] (what gvk_eval_rows wrote), target int64 [N] -> per equal-width confidence bin (i/nbins, (i+1)/nbins]
 *   count int64 [nbins], correct int64 [nbins] (top-1 hits), conf_sum f64 [nbins]; brier f64 [1] = sum_n sum_k (p_nk - 1[y_n = k])^2;
 *   nll f64 [1] = sum_n -log max(p_n,y_n, FLT_MIN).  Confidence = max_k p, prediction = its lowest index, bin = ceil(conf * nbins) - 1 (exact
 *   in double), clamped to [0, nbins).  One workgroup, every sum in row order: deterministic.  1 <= nbins <= 254; labels within [0, K). */
int gvk_tta_volumes(const float* x, const int32_t* src, const int32_t* flip, float* out, int Bout, int S, int D, int H, int W, void* stream);
int gvk_predictive_stats(const float* member_logits, float* probs, int32_t* pred, float* entropy, float* expected_entropy, float* mutual_info,
                         float* variation_ratio, float* std, int32_t* votes, int B, int S, int K, void* stream);
int gvk_calibration_bins(const float* proba, const void* target, int64_t* count, int64_t* correct, double* conf_sum, double* brier, double* nll,
                         int N, int K, int nbins, void* stream);

/* ---- bootstrap replicates of the evaluation metrics (csrc/bootstrap.hip; gaviko_amd.metrics.bootstrap / compare) ----
 * gvk_bootstrap_counts: R resamples (with replacement) of the N rows of an evaluation set, each left as the exact integers gvk_eval_rows and
 *   gvk_ovr_auc_counts leave for the full sample, with integer multiplicities w on the rows:
 *     confusion int64 [R][K][K]     confusion[b][t][p] = sum of w[b][i] over the rows with (labels[i], pred[i]) = (t, p)
 *     auc_counts int64 [R][K][3]    {sum over positives i, negatives j of w_i w_j (2 [p_i > p_j] + [p_i == p_j]), weighted n_pos, weighted n_neg}
 *   Both are written, not accumulated.  Resampling rule, for replicate b and draw n in [0, N), hash_u32 of csrc/dropout.hpp, 64-bit products:
 *     plain (stratified = 0):       j = (hash_u32(seed, b*N + n) * N) >> 32;                                         w[b][j] += 1
 *     stratified (stratified = 1):  c = labels[n], n_c = class_off[c+1] - class_off[c],
 *                                   j = class_rows[class_off[c] + ((hash_u32(seed, b*N + n) * n_c) >> 32)];           w[b][j] += 1
 *   so every replicate has N draws, the stratified one exactly n_c of them in every class, and a replicate depends on (seed, b, labels) only.
 *   The scores enter through their order alone, computed once per call by the caller (DEVICE tables, int32):
 *     order [K][N]                  the rows in ascending order of the class column (a stable sort: equal scores in row order)
 *     gstart, gend [K][N]           per sorted position, the first and one-past-last sorted position of its group of equal scores
 *     class_rows [N], class_off [K+1]   the rows grouped by label in ascending row order, and where each class starts (stratified = 1 only)
 *   labels int64 [N] within [0, K), pred int32 [N] within [0, K) (rows outside are not counted).  One 256-thread workgroup per replicate:
 *   multiplicities by 32-bit LDS atomics, per class an inclusive scan of the negatives' weights in sorted order and one pass over the
 *   positives -- O(R K N).  All integer arithmetic: bit-reproducible.  1 <= N <= GVK_BOOTSTRAP_MAX_ROWS, 2 <= K <= GVK_BOOTSTRAP_MAX_CLASSES,
 *   R >= 1 (one workgroup each; the grid's x dimension).  LDS: 8 * ceil(N / 1024) * 1024 + 4 K^2 bytes. */
enum { GVK_BOOTSTRAP_MAX_ROWS = 8192, GVK_BOOTSTRAP_MAX_CLASSES = 64 };
int gvk_bootstrap_counts(const void* labels, const int32_t* pred, const int32_t* order, const int32_t* gstart, const int32_t* gend,
                         const int32_t* class_rows, const int32_t* class_off, int64_t* confusion, int64_t* auc_counts, int N, int K, int R,
                         uint64_t seed, int stratified, void* stream);

/* ---- selective prediction and temperature scaling (csrc/selective.hip; gaviko_amd.metrics.risk_coverage / fit_temperature) ----
 * gvk_risk_coverage: the risk-coverage curve of a confidence score (Geifman & El-Yaniv, 2017) for R replicates of the N rows of an
 *   evaluation set.  labels int64 [N], pred int32 [N]: a row is WRONG when pred != label.  The scores enter through their order alone, computed
 *   once per call by the caller (DEVICE tables, int32):
 *     order [N]                     the rows by DESCENDING score (a stable sort: equal scores in row order)
 *     gend [N]                      per sorted position, one past the last sorted position of its group of equal scores
 *     class_rows [N], class_off [K+1]   the tables of gvk_bootstrap_counts, K = the number of label classes (read with resample = 1 and
 *                                   stratified = 1 only; 1 <= K <= GVK_BOOTSTRAP_MAX_CLASSES there, labels clamped into [0, K))
 *     need [Q]                      accepted-row counts within [1, N], ascending (clamped into [1, N]); 0 <= Q <= GVK_RISK_COVERAGE_MAX_NEEDS
 *   Multiplicities w on the rows: resample = 1 draws replicate b exactly as gvk_bootstrap_counts does (hash_u32(seed, b*N + n), plain or
 *   stratified, see above), so replicate b here and there is the same resample; resample = 0 requires R = 1 and gives every row w = 1.
 *   Ties are accepted together.  For the sorted groups g = 1..G: c_g = summed w of group g, e_g = summed w of its wrong rows, C_g and E_g their
 *   running sums; a group with c_g = 0 is not a threshold.  Written per replicate b, not accumulated:
 *     aurc f64 [R]                  (1/N) sum over g with c_g > 0 of c_g E_g / C_g  -- every row is charged the risk at its own threshold; for
 *                                   unit multiplicities and no ties (1/N) sum_n E_n / n.  Terms c_g E_g / C_g carry one rounding each and are
 *                                   added in a fixed order (thread t the groups starting at t, t + 256, ..; a wave's xor butterfly; the 4 waves)
 *     at int32 [R][Q][2]            (C_g, E_g) of the first group with C_g >= need[q]
 *     total int32 [R][2]            (C_G, E_G); C_G = N
 *     accepted, errors int32 [N]    resample = 0 only (else NULL; both or neither): per sorted position the (C_g, E_g) of its group
 *   One 256-thread workgroup per replicate; multiplicities by 32-bit LDS atomics, no atomics on global memory; one packed inclusive scan
 *   (w << 16 | wrong w) in tiles of 1024.  The integers are exact, aurc has the same bits on every run.  1 <= N <= GVK_BOOTSTRAP_MAX_ROWS,
 *   R >= 1 (the grid's x dimension).  LDS: 8 * ceil(N / 1024) * 1024 bytes.
 * gvk_temperature_fit: temperature scaling (Guo et al., 2017).  logits f32 [N][K], target int64 [N] within [0, K).  Minimises the mean NLL
 *   f(beta) of softmax(beta z) over beta = 1 / T in [1 / t_max, 1 / t_min]; f is convex in beta:
 *     f'(beta) = mean_n (sum_k p_nk z_nk - z_n,y)        f''(beta) = mean_n Var_{p_n}(z_n) >= 0
 *   f'(1 / t_min) <= 0: the answer is t_min; else f'(1 / t_max) >= 0: the answer is t_max (both flagged at_bound).  Otherwise safeguarded
 *   Newton from beta = 1 (clamped into the bracket): the sign of f' shrinks the bracket, a step that leaves it (or f'' = 0) is replaced by
 *   a bisection step; stop at |delta beta| <= 2^-40 beta (the step taken, or the Newton step proposed next), at f' = 0, or after 64 iterations.
 *     state f64 [8] = { T, beta, nll_before (beta = 1), nll_after, f', f'' (both at the returned beta), iterations, flags }
 *     flags: bit 0 converged (set with at_bound too: the bound is the constrained minimiser), bit 1 at_bound
 *   One 1024-thread workgroup, one launch, no host read between iterations.  All arithmetic in float64, the row maximum subtracted before
 *   exp; every sum in a fixed order (thread t the rows t, t + 1024, ..; a wave's xor butterfly; the 16 waves in order): the same bits on
 *   every run.  N >= 1, 2 <= K <= GVK_TEMPERATURE_MAX_CLASSES, 0 < t_min < t_max.  A row with a non-finite logit is the caller's contract
 *   (the fit then ends after 64 iterations with a NaN state). */
enum { GVK_RISK_COVERAGE_MAX_NEEDS = 8, GVK_TEMPERATURE_MAX_CLASSES = 64 };
int gvk_risk_coverage(const void* labels, const int32_t* pred, const int32_t* order, const int32_t* gend, const int32_t* class_rows,
                      const int32_t* class_off, const int32_t* need, double* aurc, int32_t* at, int32_t* total, int32_t* accepted,
                      int32_t* errors, int N, int K, int Q, int R, uint64_t seed, int stratified, int resample, void* stream);
int gvk_temperature_fit(const float* logits, const void* target, double* state, int N, int K, double t_min, double t_max, void* stream);

/* ---- ROC operating points of a binary reading (csrc/roc.hip; gaviko_amd.metrics.roc_analysis / roc_compare) ----
 * gvk_roc_replicates: the ROC curve of a score against a binary label for R replicates of the N rows of an evaluation set.  positive int32 [N]:
 *   a row is POSITIVE when its entry is not 0.  The scores enter through their order alone, computed once per call by the caller (DEVICE tables,
 *   int32):
 *     order [N]                     the rows by DESCENDING score (a stable sort: equal scores in row order)
 *     gend [N]                      per sorted position, one past the last sorted position of its group of equal scores
 *     strata int64 [N], class_rows [N], class_off [K+1]   the labels the stratified draw keeps the sizes of (any labelling of the rows: the
 *                                   binary label, or the K grades behind it) and the tables of gvk_bootstrap_counts for them (read with
 *                                   resample = 1 and stratified = 1 only; 1 <= K <= GVK_BOOTSTRAP_MAX_CLASSES there, strata clamped into [0, K))
 *     spec_bp [Qspec], sens_bp [Qsens]   levels in BASIS POINTS (clamped into [0, 10000]); cut_rows [Qcut]: m_q = the number of full-sample
 *                                   rows with score >= the q-th fixed threshold (clamped into [0, N]; the host finds it from the sorted
 *                                   scores).  Each list has 0 .. GVK_ROC_MAX_LEVELS entries
 *   Multiplicities w on the rows: resample = 1 draws replicate b exactly as gvk_bootstrap_counts / gvk_risk_coverage do (hash_u32(seed, b*N + n),
 *   plain or stratified, see above), so replicate b here and there is the same resample; resample = 0 requires R = 1 and gives every row w = 1.
 *   Let v_1 > v_2 > ... > v_G be the distinct scores of the full sample, tp_g / fp_g the summed w of the positive / negative rows with score
 *   v_g, TP_g / FP_g their running sums.  Point g means "call positive when score >= v_g"; point 0 is (0, 0) (call nothing positive);
 *   Pn = TP_G, Nn = FP_G.  A group of equal scores is taken together.  Written per replicate b, not accumulated:
 *     total int32 [R][2]            (Pn, Nn)
 *     auc2 int64 [R]                sum_g tp_g (2 (Nn - FP_g) + fp_g) = 2 (pairs where the positive scores higher) + (tied pairs), exact;
 *                                   AUC = auc2 / (2 Pn Nn), formed by the host
 *     ap f64 [R]                    average precision (the step definition of sklearn), DIVIDED BY Pn IN THE KERNEL:
 *                                   (1 / Pn) sum over g with tp_g > 0 of tp_g TP_g / (TP_g + FP_g); NaN when Pn = 0.  Each product is an exact
 *                                   integer below 2^26 and takes one rounding in the division; the terms are added in a fixed order (thread t
 *                                   the groups starting at t, t + 256, ..; a wave's xor butterfly; the 4 waves), then one division
 *     at_spec int32 [R][Qspec][2]   (TP_g, FP_g) of the LAST point g in 0..G with (Nn - FP_g) * 10000 >= spec_bp[q] * Nn: the sensitivity at
 *                                   specificity >= spec_bp[q] / 10000.  Exact in 32-bit integers; point 0 always qualifies
 *     at_sens int32 [R][Qsens][2]   (TP_g, FP_g) of the FIRST point g in 0..G with TP_g * 10000 >= sens_bp[q] * Pn: the specificity at
 *                                   sensitivity >= sens_bp[q] / 10000.  Point G always qualifies
 *     at_cut int32 [R][Qcut][2]     the running (TP, FP) over the first m_q sorted positions; m_q = 0 gives (0, 0)
 *     youden int32 [R][3]           (TP_g, FP_g, s_g) of the point maximising TP_g * Nn - FP_g * Pn over the points 1..G that a draw reached
 *                                   (tp_g + fp_g > 0); on a tie the smallest g.  s_g = the first sorted position of the group: the threshold
 *                                   is score[order[s_g]]
 *     tp, fp int32 [N]              resample = 0 only (else NULL; both or neither): per sorted position the (TP_g, FP_g) of its group
 *   One 256-thread workgroup per replicate; multiplicities by 32-bit LDS atomics, no atomics on global memory; one packed inclusive scan
 *   (positive ? w << 16 : w) in tiles of 1024.  The integers are exact, ap has the same bits on every run.  1 <= N <= GVK_BOOTSTRAP_MAX_ROWS,
 *   R >= 1 (the grid's x dimension).  LDS: 8 * ceil(N / 1024) * 1024 bytes. */
enum { GVK_ROC_MAX_LEVELS = 8 };
int gvk_roc_replicates(const void* strata, const int32_t* positive, const int32_t* order, const int32_t* gend, const int32_t* class_rows,
                       const int32_t* class_off, const int32_t* spec_bp, const int32_t* sens_bp, const int32_t* cut_rows, int32_t* total,
                       int64_t* auc2, double* ap, int32_t* at_spec, int32_t* at_sens, int32_t* at_cut, int32_t* youden, int32_t* tp, int32_t* fp,
                       int N, int K, int Qspec, int Qsens, int Qcut, int R, uint64_t seed, int stratified, int resample, void* stream);

/* ---- split-conformal prediction sets (csrc/conformal.hip; gaviko_amd.metrics.conformal_scores / conformal_calibrate / conformal_evaluate) ----
 * gvk_conformal_scores: proba f32 [N][K] -> scores f32 [K][N] (CLASS-MAJOR: gvk_conformal_splits reads a class column over consecutive rows).
 *   Rank of class k in its row, 0-based:  r_k = #{j : p_j > p_k or (p_j == p_k and j < k)}  (ties go to the lower class index); pi(r) = the
 *   class of rank r.  Every operation below is ONE fp32 rounding, never contracted into an FMA (a numpy float32 restatement gives the bits):
 *     kind GVK_CONFORMAL_LAC  (Sadinle et al., 2019):       s_k = 1 - p_k
 *     kind GVK_CONFORMAL_APS  (Romano et al., 2020):        c_0 = 0, c_{r+1} = c_r + p_pi(r), added sequentially in rank order;
 *                                                           randomized = 0: s_pi(r) = c_{r+1};  randomized = 1: s_pi(r) = c_r + (u_n * p_pi(r))
 *                                                           with one u_n = float(hash_u32(seed, n) >> 8) * 2^-24 per row (hash_u32 of
 *                                                           csrc/dropout.hpp; u_n in [0, 1), exact)
 *     kind GVK_CONFORMAL_RAPS (Angelopoulos et al., 2021):  s = aps + (lam * float(max(0, r + 1 - k_reg))),  lam >= 0, k_reg >= 0
 *   One wave per row, one class per lane, no atomics.  N >= 1, 2 <= K <= GVK_CONFORMAL_MAX_CLASSES; randomized = 1 needs aps or raps; seed,
 *   k_reg and lam are read by the kinds that name them.  NaN probabilities are the caller's contract.
 * gvk_conformal_splits: R random calibration/test splits of the N rows of an evaluation set, one 256-thread workgroup per replicate b.
 *   scores f32 [K][N] (as written above), labels int64 [N] within [0, K) (clamped), alphas f64 [Q] miscoverage levels within (0, 1), all on
 *   the DEVICE, and two DEVICE tables computed once per call by the caller (int32):
 *     order [N]                     the rows grouped by segment, inside a segment ascending by TRUE-class score scores[labels[i]][i] (a stable
 *                                   sort: equal scores in row order).  G = 1: one segment (marginal); G = K: segment = label (class-conditional,
 *                                   "Mondrian")
 *     seg_off [G+1]                 where each segment starts in `order`
 *   Split rule:  key_i = (hash_u32(seed, b*N + i) & ~0x1FFF) | i  -- distinct, the row index fits the low 13 bits -- and the calibration rows of
 *   replicate b are the n_cal rows with the smallest keys (numpy: argsort(keys)[:n_cal]); the rest are test rows.  n_cal = N: every row
 *   calibrates, no test rows (how a predictor is calibrated on a whole set).  A replicate depends on (seed, b, N, n_cal) only.
 *   Threshold of segment g with n_g calibration rows at level q, in float64 with exactly this expression:
 *     m = (int)ceil((double)(n_g + 1) * (1.0 - alphas[q]))   (at least 1);   m > n_g: qhat = +inf, qpos = -1;   else qhat = the true-class score of
 *     the m-th calibration row of the segment in sorted order, qpos = its position in `order`
 *   Every test row i and level q:  size = #{k : scores[k][i] <= qhat[q][g(k)]},  covered = scores[y_i][i] <= qhat[q][g(y_i)],  g(k) = 0 (G = 1) or
 *   k (G = K).  Written per replicate, never accumulated, int32:
 *     qpos [R][Q][G]                see above
 *     n_seg [R][G]                  n_g
 *     size_hist [R][Q][K+1]         test rows by set size
 *     covered_by_size [R][Q][K+1]   covered test rows by set size
 *     class_test [R][K]             test rows by label
 *     class_covered [R][Q][K]       covered test rows by label
 *   The selection is a 4-pass radix select of the n_cal-th smallest key, the order statistic one inclusive scan of the membership flags over
 *   `order` in tiles of 1024, the histograms LDS integer atomics; no atomics on global memory: exact integers, the same on every run.
 *   1 <= N <= GVK_BOOTSTRAP_MAX_ROWS, 2 <= K <= GVK_CONFORMAL_MAX_CLASSES, 1 <= Q <= GVK_CONFORMAL_MAX_LEVELS, G in {1, K}, 1 <= n_cal <= N,
 *   R >= 1 (the grid's x dimension).  LDS: 8 * ceil(N / 1024) * 1024 + 14176 bytes. */
enum { GVK_CONFORMAL_MAX_CLASSES = 64, GVK_CONFORMAL_MAX_LEVELS = 8 };
enum { GVK_CONFORMAL_LAC = 0, GVK_CONFORMAL_APS = 1, GVK_CONFORMAL_RAPS = 2 };
int gvk_conformal_scores(const float* proba, float* scores, int N, int K, int kind, int randomized, uint64_t seed, int k_reg, float lam,
                         void* stream);
int gvk_conformal_splits(const float* scores, const void* labels, const int32_t* order, const int32_t* seg_off, const double* alphas,
                         int32_t* qpos, int32_t* n_seg, int32_t* size_hist, int32_t* covered_by_size, int32_t* class_test, int32_t* class_covered,
                         int N, int K, int Q, int G, int n_cal, int R, uint64_t seed, void* stream);

/* ---- feature embeddings and kNN probes (csrc/features.hip; gaviko_amd/features.py) ----
 * All fp32, no atomics, every sum in a fixed order: two runs are bit-identical.
 * gvk_token_pool: out f32 [B][C], out[b][c] = (1/R) sum_{r in [r0, r0+R)} g[b][r][c] of a token stream g f32 [B][T][C] (row pitch C).
 *   1 <= R <= T - r0, C % 4 == 0, C <= 1024.  R = 1 copies row r0 bit for bit (no division).  16 waves per (64-column tile, sample): wave w adds
 *   the rows w, w+16, ... in order, the 16 partials are added as a fixed binary tree -- the order depends on R alone.  Bytes: B*R*C*4 read.
 * gvk_l2_normalize_rows: y[n] = x[n] / max(||x[n]||, eps) for x f32 [N][C]; y == x (in place) or disjoint; norm f32 [N] (optional) receives
 *   ||x[n]||.  One wave per row, the squares added per lane in column order, then the xor butterfly.
 * gvk_feature_topk: queries q f32 [Nq][C], bank g f32 [Ng][C] -> idx int32 [Nq][k], score f32 [Nq][k], best first.
 *     metric 0: score = q . g, larger is better.  metric 1: score = (||q||^2 + ||g||^2) - 2 q . g (squared L2), smaller is better.
 *   An exact tie of the fp32 score goes to the LOWER bank index.  exclude int32 [Nq] (optional): one bank index per query that is skipped
 *   (-1: none).  NaN scores are never selected; a slot with no candidate left holds index -1.
 *   1 <= k <= 32, k <= Ng - (exclude ? 1 : 0), C % 4 == 0, C <= 1024, Nq, Ng >= 1, Nq * Ng < 2^31.
 *   Products on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), 16 queries x 16 bank rows per tile, the contraction in an
 *   order that depends on C alone: a score does not depend on Nq, Ng, its tile or the slab split.  The bank is cut into `nslabs` slabs of
 *   16-row tiles over workgroups (grid = query tiles x slabs, so a handful of queries still fills the device); every slab keeps a sorted
 *   top-k per query, a second kernel merges the slab lists by the same (score, index) rule -- the result does not depend on nslabs.
 *   nslabs must be a value gvk_feature_topk_slabs(Nq, Ng, want) returns (want <= 0: the default; want > 0: the nearest valid count, at most
 *   128); scratch: 2 * Nq * nslabs * k 32-bit words.
 * gvk_knn_vote: idx / score [Nq][k] (as written above), labels int32 [Ng] -> probs f32 [Nq][K], pred int32 [Nq] (argmax, lowest class on a tie).
 *   mode 0: probs[c] = #{j: label[idx_j] == c} / k.  mode 1: w_j = exp((score_j - score_0) / temperature), probs[c] = sum_{j: label = c} w_j /
 *   sum_j w_j, summed in rank order (for metric 1 pass -distance).  Weights and sums in double, one rounding at the store.  An index outside
 *   [0, Ng) or a label outside [0, K) has no vote (the caller rejects such labels).  1 <= k <= 32, 2 <= K <= 256.
 * gvk_class_means: x f32 [N][C], labels int32 [N] -> mean f32 [K][C], count int32 [K]; every class summed in row order; an empty class
 *   gives count 0 and a row of exact zeros. */
typedef struct gvk_feature_topk_desc {
  const float* q; const float* g; const int32_t* exclude; int32_t* idx; float* score; void* scratch;
  int32_t Nq, Ng, C, k, metric, nslabs;
  int64_t scratch_words;
} gvk_feature_topk_desc;
int gvk_token_pool(const float* g, float* out, int B, int T, int C, int r0, int R, void* stream);
int gvk_l2_normalize_rows(const float* x, float* y, float* norm, int N, int C, float eps, void* stream);
int gvk_feature_topk_slabs(int Nq, int Ng, int want);
int gvk_feature_topk(const gvk_feature_topk_desc* d, void* stream);
int gvk_knn_vote(const int32_t* idx, const float* score, const int32_t* labels, float* probs, int32_t* pred, int Nq, int Ng, int k, int K, int mode,
                 float temperature, void* stream);
int gvk_class_means(const float* x, const int32_t* labels, float* mean, int32_t* count, int N, int C, int K, void* stream);

/* ---- raw volumes of any shape and spacing onto the model grid (csrc/conform.hip; gaviko_amd.data.Conform) ----
 * torchio's first stage (Resample to a spacing / Resize, then CropOrPad) for a RAGGED batch: `data` holds B float32 volumes of unequal
 * shape n_b = (n0, n1, n2), each in [D][H][W] order, sample b starting at element offset off_b (any alignment); the output is the uniform
 * out [B][D][H][W].  Per sample and per array axis a the whole geometry is ONE banded table built on the host in float64 and rounded to
 * float32 once (data.conform_tables): output index q reads the inputs start[q] .. start[q] + K - 1 with weights[q][0..K), or -- inside[q] == 0
 * -- lies in the padding.  The tables of the three axes are concatenated: start / inside int32 [B][D + H + W] (offsets 0, D, D + H),
 * weights float32 [B][D + H + W][T], T <= GVK_CONFORM_MAX_TAPS the row length (a sample's own band K <= T is in its meta rows).
 * gvk_ragged_minmax: partials [B][gvk_minmax_partials()] = the (min, max) slab pairs of the counts[b] elements at data + offsets[b], the
 *   layout of gvk_volume_minmax (offsets, counts int64 [B], DEVICE tables); scalar loads, no alignment assumed.  Exact.
 * gvk_conform_volumes: the contraction is separable, so it runs as npass <= 3 streaming passes, one contracted axis each, lanes along W in
 *   every pass.  The caller plans them (ops.conform_volumes): per pass p and sample b a meta row of 16 int32
 *     { live, src_sel (0 data, 1 scratch), dst_sel (0 scratch, 1 out), mode[3], in_dims[3], out_dims[3], contracted axis or -1, K, 0, 0 }
 *   with mode 0 = untouched so far (identity), 1 = gathered in this pass (out[q] = in[start[q]]: a move of 32-bit words), 2 = contracted in
 *   this pass, 3 = done in an earlier pass (already on the output grid), and src_off / dst_off int64 [3][B] the element offsets of the
 *   sample inside the selected buffers.  An axis whose rows are all single taps of weight 1 is gathered, never multiplied: a batch that is
 *   only cropped, padded or already conforming comes out bit for bit in one pass.  A contracted element is
 *   v = w[0] x[0]; v = fmaf(w[t], x[t], v) for t = 1..K-1 (one rounding per tap), stored as float32 between passes.  An output voxel that is
 *   outside on any axis touched so far is written as the pad value in every pass, so the padding is exact: pad_value, or with pad_min != 0
 *   the sample's own minimum reduced on the device from partials (gvk_ragged_minmax).  The device tables are not read by the host: every
 *   index they imply (start[q] + K <= n on inside rows, the offsets) must have been checked by the caller.  pass_dims[p] = the largest
 *   out_dims over the live samples of pass p (the grid).  No atomics: the same bits on every run.  64-bit element offsets throughout.
 *   Bytes: every pass reads its input once and writes its output once; with the axis of largest reduction first the intermediates are
 *   the smallest possible. */
enum { GVK_CONFORM_MAX_TAPS = 16, GVK_CONFORM_META = 16 };
typedef struct gvk_conform_desc {
  const float* data; float* scratch; float* out; const int64_t* src_off; const int64_t* dst_off; const int32_t* meta; const int32_t* start;
  const int32_t* inside; const float* weights; const float* partials;
  int32_t B, D, H, W, T, npass, pad_min, p0d0, p0d1, p0d2, p1d0, p1d1, p1d2, p2d0, p2d1, p2d2;
  float pad_value;
} gvk_conform_desc;
int gvk_ragged_minmax(const float* data, const int64_t* offsets, const int64_t* counts, float* partials, int B, void* stream);
int gvk_conform_volumes(const gvk_conform_desc* d, void* stream);

/* ---- out-of-distribution statistics (csrc/ood.hip; gaviko_amd/ood.py) ----
 * fp32 in, no atomics, every sum in a fixed order: two runs are bit-identical.  C % 4 == 0, C <= 1024 as in the feature kernels; x, mean,
 * q, W and m 16-byte aligned.
 * gvk_scatter_matrix: x f32 [N][C], labels int32 [N] or NULL, mean f32 [K][C].  With d_i = fl32(x_i - mean[labels_i]) (row 0 of mean for every
 *   row when labels is NULL) it writes
 *     S f64 [C][C] = sum_i d_i d_i^T (NOT divided),   r4 f64 [1] = sum_i (||d_i||^2)^2,   count int32 [K] = rows per label.
 *   A label outside [0, K) contributes nothing and is not counted (the caller rejects such labels).  1 <= K <= 65535, N >= 1.
 *   Products on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  The rows are cut into chunks of 64 rows at absolute row
 *   indices (chunk c = rows [64 c, 64 c + 64)): inside a chunk an entry is one chain of fp32 fmas in row order, the chunk sums are then added in
 *   double, in chunk order inside a slab of consecutive chunks and in slab order over the slabs.  ||d_i||^2 is summed in fp32 (per lane the
 *   columns 4 l .. 4 l + 3, 4 l + 256 .., then the xor butterfly), squared and accumulated in double: per chunk in row order, then thread t
 *   of one workgroup adds the chunks t, t + 256, .. and the 256 sums are folded in halves -- an order that depends on N alone.  Only the 64 x 64 tiles on and above
 *   the diagonal are computed and each is written twice from the same double: S == S^T bit for bit.  Grid = tile pairs x slabs; with
 *   nt = ceil(C / 64), npairs = nt (nt + 1) / 2, nchunks = ceil(N / 64):  want = min(nchunks, ceil(512 / npairs)),  cps = ceil(nchunks / want),
 *   nslabs = ceil(nchunks / cps) -- a function of (N, C) alone.  scratch: (nslabs * npairs * 4096 + nchunks) * 8 bytes, 8-byte aligned.
 *   Rows past N are never read.
 * gvk_mahalanobis: q f32 [Nq][C], W f32 [C][C] (dense whitening matrix, z = W v), m f32 [K][C] -> d2 f32 [Nq][K],
 *     d2[n][k] = sum_j ( (W q_n)_j - (W m_k)_j )^2 ,   (W v)_j = sum_c W[j][c] v[c] on v_mfma_f32_16x16x4_f32 in column order,
 *   the queries and the centres whitened by the same chain of fmas (q_n == m_k bit for bit gives exactly 0), the differences of the whitened
 *   coordinates formed, squared and added in fp32: never the ||z||^2 + ||m||^2 - 2 z.m form, d2 >= 0 always.  The whitened rows stay on the
 *   chip: a workgroup of eight waves holds 16 queries, wave w walks the coordinate chunks [16 t, 16 t + 16), t = w, w + 8, .., and keeps K
 *   running sums per query; a lane adds its coordinates in chunk order, the 16 lanes of a query meet in the xor butterfly (1, 2, 4, 8), the
 *   eight waves are added in wave order.  The order depends on C alone: a row's result does not depend on Nq, its tile or the grid.
 *   1 <= K <= 32, Nq >= 1.  Rows past Nq are never read.  Cost: ceil(Nq / 16) workgroups, each reading all of W (from L2) and whitening the
 *   K centres again: bound by the W traffic, and CUs stay idle below Nq of about 4096.
 * gvk_logit_scores: logits f32 [N][K], temperature T > 0 -> out f32 [N][4] = { max softmax probability, max logit, T logsumexp(z / T),
 *   entropy of softmax(z) in nats with 0 log 0 = 0 }.  One wave per row, computed in double shifted by the row maximum, one rounding at the
 *   store; nothing overflows for finite logits, the entropy is >= 0.  2 <= K <= 256, N >= 1. */
int gvk_scatter_matrix(const float* x, const int32_t* labels, const float* mean, double* S, double* r4, int32_t* count, void* scratch,
                       int64_t scratch_bytes, int N, int C, int K, void* stream);
int gvk_mahalanobis(const float* q, const float* W, const float* m, float* d2, int Nq, int C, int K, void* stream);
int gvk_logit_scores(const float* logits, float* out, int N, int K, float temperature, void* stream);

#ifdef __cplusplus
}
#endif
#endif
