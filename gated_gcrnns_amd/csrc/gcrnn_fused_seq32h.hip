// Instantiations and launcher of the wide forward WITH the output head (gcrnn_fused_seq32.h, VAR bit 3): inference of cell + Linear(F -> 1)
// shared by all nodes (the regression model's `multipMlp` head with one output) as ONE launch -- the state hand-over of the state-scratch
// variant, y [B][T][N] fp32 instead of H. A translation unit of its own, compiled beside the others.
#include "gcrnn_fused_step.h"
#define GCRNN_SEQ32_STAMP_READER_NAME gcrnn_debug_read_seq32h_stamps      // (diagnostic builds: this unit's own stamp array and reader)
#include "gcrnn_fused_seq32.h"

template <int K, int HS, int XS, int VAR, bool GATED, bool R1>
static int seq32h_launch_v(const Seq32Args& sa, size_t lds, hipStream_t st) {
  static_assert((VAR & 14) == 12, "output head: on the state scratch, without the user-layout output");
  auto sk = fused_seq32_kernel<K, HS, XS, VAR, 0, GATED, R1>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(sk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  // one workgroup per CU: the scratch is sized by this grid. Self-start: one workgroup per SEQUENCE (its start-up phase runs in front of the
  // kernel's tables) -- beyond the persistent grid they start as CUs free up, and the entry point has put their scratch into the work buffer
  sk<<<(unsigned)((sa.B < gcrnn_persistent_grid() || sa.self_start) ? sa.B : gcrnn_persistent_grid()), STHREADS, lds, st>>>(sa);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <int K, int HS, int XS>
static int seq32h_launch(const Seq32Args& sa, bool inline_pack, hipStream_t st) {
  if (!sa.y0 || !sa.head_w || (HS > 1 && !sa.scr)) return GCRNN_ERR_NULL_POINTER;
  const size_t lds = Seq32Map<K, HS, XS>::lds_bytes_head(sa.entries, inline_pack, sa.r1a != nullptr);
  if (!lds) return GCRNN_ERR_UNSUPPORTED;
  if (sa.gi0) {      // time-gated recurrence: the gate pre-pass has laid out X
    if (inline_pack) return GCRNN_ERR_BAD_SHAPE;
    return sa.r1a ? seq32h_launch_v<K, HS, XS, 12, true, true>(sa, lds, st) : seq32h_launch_v<K, HS, XS, 12, true, false>(sa, lds, st);
  }
  if (sa.r1a) return inline_pack ? seq32h_launch_v<K, HS, XS, 13, false, true>(sa, lds, st) : seq32h_launch_v<K, HS, XS, 12, false, true>(sa, lds, st);
  return inline_pack ? seq32h_launch_v<K, HS, XS, 13, false, false>(sa, lds, st) : seq32h_launch_v<K, HS, XS, 12, false, false>(sa, lds, st);
}

#define GCRNN_SEQ32H_CASES(X_) \
  X_(5, 2, 2) X_(4, 2, 2) X_(3, 2, 2) X_(2, 2, 2) X_(5, 2, 1) X_(4, 2, 1) X_(3, 2, 1) X_(2, 2, 1) X_(5, 1, 1) X_(4, 1, 1) X_(3, 1, 1) X_(2, 1, 1)

// LDS bytes of the head variant (0: no such instantiation, or no room)
size_t gcrnn_seq32h_lds(int64_t F, int64_t G, int64_t K, int64_t entries, bool inline_pack, bool r1) {
#define GCRNN_SEQ32H_CASE(KK, HH, XX) if (K == KK && F == 32 * HH && G == 32 * XX) return Seq32Map<KK, HH, XX>::lds_bytes_head(entries, inline_pack, r1);
  GCRNN_SEQ32H_CASES(GCRNN_SEQ32H_CASE)
#undef GCRNN_SEQ32H_CASE
  return 0;
}

// the persistent forward with the head (gcrnn_fused_seq32.hip, gcrnn_fused_forward_wide_head_bf16, dispatches here)
int gcrnn_seq32h_forward(const Seq32Args& sa, int K, int HS, int XS, bool inline_pack, hipStream_t st) {
#define GCRNN_SEQ32H_CASE(KK, HH, XX) if (K == KK && HS == HH && XS == XX) return seq32h_launch<KK, HH, XX>(sa, inline_pack, st);
  GCRNN_SEQ32H_CASES(GCRNN_SEQ32H_CASE)
#undef GCRNN_SEQ32H_CASE
  return GCRNN_ERR_UNSUPPORTED;
}
