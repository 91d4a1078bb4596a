// Host side of gvk_attention_fwd / gvk_attention_bwd (include/gaviko_hip.h), shared by attention_fwd.hip, attention_bwd.hip and
// attention_f32.hip: the one validation of a gvk_attention_desc, the key-tile choice, the dropout constants of the kernels, and the
// fp32 launchers the two entry points (which live in the bf16 sources) hand an f32 descriptor to.
#pragma once
#include "common.hpp"
#include "dropout.hpp"
#include "../../include/gaviko_hip.h"

namespace gvk {

// attention-probability dropout (vision_transformer.py:68, live for the unfrozen-backbone methods): the softmax statistics are taken
// of the undropped scores, the dropped and rescaled P feeds the P.V product; mask element (b*H + head, query, key) -- dropout.hpp.
// thresh = 0: off.  Both precisions take the same constants, so they drop the same elements.
struct AttnDrop { unsigned long long seed; const unsigned long long* seed_ptr; unsigned int thresh; float inv_keep; };

inline AttnDrop attn_drop(const gvk_attention_desc& d) {
  return {d.seed, (const unsigned long long*)d.seed_ptr, drop_threshold_u32(d.drop_p), d.drop_p > 0.f ? 1.f / (1.f - d.drop_p) : 1.f};
}

// key / query tile of the bf16 flash kernels: the size that pads the sequence less (T = 1033: 11 x 96 = 1056 against 9 x 128 = 1152),
// ties go to the larger tile; GAVIKO_HIP_ATTN_KB=96|128 forces one (test hook; read per launch, so one process can run both)
inline int attn_key_tile(int T) {
  const char* e = getenv("GAVIKO_HIP_ATTN_KB");
  const int forced = e ? atoi(e) : 0;
  if (forced == 96 || forced == 128) return forced;
  return ((T + 95) / 96 * 96 < (T + 127) / 128 * 128) ? 96 : 128;
}

// Every check of a descriptor that does not depend on a kernel's own layout (the one-pass backward checks its workspace itself).
// Contradictory requests are refused, never resolved by precedence: a caller that wants one (ops.attention_bwd) applies it first.
inline int attn_validate(const gvk_attention_desc* d, bool bwd, const char* name) {
  GVK_REQUIRE(d, "%s: null descriptor", name);
  GVK_REQUIRE(d->qkv && d->out && (!bwd || (d->dout && d->lse && d->delta && d->dqkv)), "%s: null pointer", name);
  GVK_REQUIRE(d->B > 0 && d->T > 0 && d->H > 0, "%s: empty shape", name);
  const int per16 = d->f32 ? 4 : 8;                 // elements in 16 bytes: the row pitch is a multiple of 16 bytes
  GVK_REQUIRE(d->ld_qkv >= 3 * d->H * 64 && d->ld_qkv % per16 == 0 && d->ld_out >= d->H * 64 && d->ld_out % per16 == 0,
              "%s: head dim is fixed at 64; ld_qkv=%d ld_out=%d inconsistent with H=%d (16-byte rows)", name, d->ld_qkv, d->ld_out, d->H);
  GVK_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f && (d->drop_p == 0.f || d->seed_ptr != nullptr), "%s: drop_p in [0,1) and a seed word", name);
  GVK_REQUIRE(d->drop_p == 0.f || (int64_t)d->T * d->T < (int64_t)1 << 32, "%s: the dropout mask index (query*T + key) is 32-bit", name);
  GVK_REQUIRE(d->f32 || (int64_t)d->B * d->T * d->ld_qkv * 2 < (int64_t)1 << 31,
              "%s: the qkv tensor must stay below 2 GiB (32-bit buffer offsets)", name);
  if (!bwd) {
    GVK_REQUIRE(!d->ws, "%s: ws given to the forward (the workspace belongs to the one-pass backward)", name);
    return 0;
  }
  GVK_REQUIRE(d->need_rows >= 0 && d->need_rows <= d->T, "%s: need_rows=%d outside [0, T=%d]", name, d->need_rows, d->T);
  GVK_REQUIRE(!(d->need_rows > 0 && d->drop_p > 0.f), "%s: need_rows conflicts with drop_p > 0 (the dropout kernels write every row)", name);
  GVK_REQUIRE(!(d->need_rows > 0 && d->ws), "%s: need_rows conflicts with ws (the one-pass kernel writes every row)", name);
  GVK_REQUIRE(!(d->ws && d->drop_p > 0.f), "%s: ws conflicts with drop_p > 0 (the one-pass kernel has no dropout)", name);
  GVK_REQUIRE(!(d->f32 && (d->ws || d->need_rows > 0)), "%s: ws and need_rows conflict with f32 (fp32 has the plain two-pass backward only)", name);
  return 0;
}

// attention_f32.hip: a validated descriptor with f32 = 1
int launch_attn_fwd_f32(const gvk_attention_desc& d, hipStream_t stream);
int launch_attn_bwd_f32(const gvk_attention_desc& d, hipStream_t stream);

}  // namespace gvk
