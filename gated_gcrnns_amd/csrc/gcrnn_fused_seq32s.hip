// Instantiations and launcher of the wide forward WITHOUT a state image (gcrnn_fused_seq32.h, VAR bit 2): inference with the user-layout
// output, where the only state bytes the launch reads back live in a per-workgroup scratch in slot order. A translation unit of its own: the
// variant doubles the VAR 2 / 3 instantiations of the header, and the units are compiled side by side.
#include "gcrnn_fused_step.h"
#define GCRNN_SEQ32_STAMP_READER_NAME gcrnn_debug_read_seq32s_stamps      // (diagnostic builds: this unit's own stamp array and reader)
#include "gcrnn_fused_seq32.h"

template <int K, int HS, int XS, int VAR, bool GATED, bool R1>
static int seq32s_launch_v(const Seq32Args& sa, size_t lds, hipStream_t st) {
  static_assert((VAR & 6) == 6, "state scratch: with the user-layout output");
  auto sk = fused_seq32_kernel<K, HS, XS, VAR, 0, GATED, R1>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(sk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  // one workgroup per CU: the scratch is sized by this grid. Self-start: one workgroup per SEQUENCE (its start-up phase runs in front of the
  // kernel's tables) -- beyond the persistent grid they start as CUs free up, and forward_wide_impl has put their scratch into the work buffer
  sk<<<(unsigned)((sa.B < gcrnn_persistent_grid() || sa.self_start) ? sa.B : gcrnn_persistent_grid()), STHREADS, lds, st>>>(sa);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// the VAR 7 forward on resident tiles (gcrnn_fused_seq32r.hip): its LDS bytes -- 0 when it does not take the launch -- and its launcher
size_t gcrnn_seq32r_lds(int K, int HS, int XS, int64_t entries, bool r1, int* rt);
int gcrnn_seq32r_forward(const Seq32Args& sa, int K, int XS, int rt, size_t lds, hipStream_t st);

template <int K, int HS, int XS>
static int seq32s_launch(const Seq32Args& sa, bool inline_pack, size_t lds, hipStream_t st) {
  if (!sa.a1 || (HS > 1 && !sa.scr)) return GCRNN_ERR_NULL_POINTER;
  if (HS > 1 && inline_pack && !sa.gi0) {      // un-gated, as the module issues it: resident tiles where the map has room for them
    int rt = 0;
    const size_t ldsr = gcrnn_seq32r_lds(K, HS, XS, sa.entries, sa.r1a != nullptr, &rt);
    if (ldsr) return gcrnn_seq32r_forward(sa, K, XS, rt, ldsr, st);
  }
  if (sa.gi0) {      // time-gated recurrence: the gate pre-pass has laid out X
    if (inline_pack) return GCRNN_ERR_BAD_SHAPE;
    return sa.r1a ? seq32s_launch_v<K, HS, XS, 6, true, true>(sa, lds, st) : seq32s_launch_v<K, HS, XS, 6, true, false>(sa, lds, st);
  }
  if (sa.r1a) return inline_pack ? seq32s_launch_v<K, HS, XS, 7, false, true>(sa, lds, st) : seq32s_launch_v<K, HS, XS, 6, false, true>(sa, lds, st);
  return inline_pack ? seq32s_launch_v<K, HS, XS, 7, false, false>(sa, lds, st) : seq32s_launch_v<K, HS, XS, 6, false, false>(sa, lds, st);
}

// the persistent forward on the state scratch (gcrnn_fused_seq32.hip, gcrnn_fused_forward_wide_scratch_bf16, dispatches here)
int gcrnn_seq32s_forward(const Seq32Args& sa, int K, int HS, int XS, bool inline_pack, size_t lds, hipStream_t st) {
#define GCRNN_SEQ32S_CASE(KK, HH, XX) if (K == KK && HS == HH && XS == XX) return seq32s_launch<KK, HH, XX>(sa, inline_pack, lds, st);
  GCRNN_SEQ32S_CASE(5, 2, 2) GCRNN_SEQ32S_CASE(4, 2, 2) GCRNN_SEQ32S_CASE(3, 2, 2) GCRNN_SEQ32S_CASE(2, 2, 2)
  GCRNN_SEQ32S_CASE(5, 2, 1) GCRNN_SEQ32S_CASE(4, 2, 1) GCRNN_SEQ32S_CASE(3, 2, 1) GCRNN_SEQ32S_CASE(2, 2, 1)
  GCRNN_SEQ32S_CASE(5, 1, 1) GCRNN_SEQ32S_CASE(4, 1, 1) GCRNN_SEQ32S_CASE(3, 1, 1) GCRNN_SEQ32S_CASE(2, 1, 1)
#undef GCRNN_SEQ32S_CASE
  return GCRNN_ERR_UNSUPPORTED;
}
