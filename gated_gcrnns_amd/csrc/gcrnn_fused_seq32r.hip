// Instantiations and launcher of the wide forward with RESIDENT TILES (gcrnn_fused_seq32.h, template argument RT): the un-gated inference
// forward as the module issues it (VAR 7: inline pack, user-layout output, state scratch; uniform-weight or rank-1 graph) at F = 64, where
// chunk 0 of h_t is read back one step later. The tap weights sit in a ring of three taps, and in the bytes that frees the first RT tiles
// of every wave keep their chunk-0 fragment in LDS instead of the scratch. A translation unit of its own, compiled beside the others.
//
// Not here, on purpose: the time-gated recurrence (VAR 6, GATED), the caller-packed form (VAR 6) and the output head (VAR 12 / 13) keep
// RT = 0 and one chunk's taps in LDS, as do F = 32 (nothing is re-read), the state-image launches, the hand-allocated hop and split batches.
#include <cstdlib>
#include "gcrnn_fused_step.h"
#define GCRNN_SEQ32_STAMP_READER_NAME gcrnn_debug_read_seq32r_stamps      // (diagnostic builds: this unit's own stamp array and reader)
#include "gcrnn_fused_seq32.h"

// RT = 2 or 3: the largest that fits beside the graph's column words. K = 5, F = G = 64: 3 x 8 KB ring + 2 x 8 KB block = the 40 KB that
// held one chunk's five taps; the third tile takes 8 KB of what the map left spare (the bench graph: 10.4 KB; not with rank-1 factor tables).

// GCRNN_SEQ32_RESIDENT (read at every call): 0 = the RT = 0 launch of the same binary (same-binary A/B and the bit-identity tests),
// 2 = at most two tiles (A/B of the third)
static int seq32_resident_max() {
  const char* e = getenv("GCRNN_SEQ32_RESIDENT");
  if (!e) return 3;
  return e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 3);
}

template <int K, int XS, bool R1, int RT>
static int seq32r_launch_v(const Seq32Args& sa, size_t lds, hipStream_t st) {
  auto sk = fused_seq32_kernel<K, 2, XS, 7, 0, false, R1, false, RT>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(sk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  // (the grid of the state-scratch launcher: one workgroup per CU, or -- self-start -- per sequence)
  sk<<<(unsigned)((sa.B < gcrnn_persistent_grid() || sa.self_start) ? sa.B : gcrnn_persistent_grid()), STHREADS, lds, st>>>(sa);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// LDS bytes of the resident form and its tile count (0: no such instantiation, the switch is off, or the graph's column words leave no
// room for the block)
size_t gcrnn_seq32r_lds(int K, int HS, int XS, int64_t entries, bool r1, int* rt) {
  *rt = 0;
  const int mx = seq32_resident_max();
  if (HS != 2 || mx == 0) return 0;
  if (K == 4 && XS == 2 && r1) return 0;      // (hipcc spills two vector registers in that one instantiation, none at RT = 0: it keeps RT = 0)
#define GCRNN_SEQ32R_CASE(KK, XX) \
  if (K == KK && XS == XX) { \
    size_t l = mx >= 3 ? Seq32Map<KK, 2, XX, 3>::lds_bytes(entries, true, r1) : 0; \
    if (l) { *rt = 3; return l; } \
    l = Seq32Map<KK, 2, XX, 2>::lds_bytes(entries, true, r1); \
    if (l) *rt = 2; \
    return l; \
  }
  GCRNN_SEQ32R_CASE(5, 2) GCRNN_SEQ32R_CASE(4, 2) GCRNN_SEQ32R_CASE(3, 2) GCRNN_SEQ32R_CASE(2, 2)
  GCRNN_SEQ32R_CASE(5, 1) GCRNN_SEQ32R_CASE(4, 1) GCRNN_SEQ32R_CASE(3, 1) GCRNN_SEQ32R_CASE(2, 1)
#undef GCRNN_SEQ32R_CASE
  return 0;
}

extern "C" int gcrnn_fused_forward_wide_resident_tiles(int64_t F, int64_t G, int64_t K, int64_t entries, int rank1) {
  if (F != 64 || G <= 0 || G % 32 || entries <= 0) return 0;
  int rt = 0;
  gcrnn_seq32r_lds((int)K, 2, (int)(G / 32), entries, rank1 != 0, &rt);
  return rt;
}

// the VAR 7 forward on resident tiles (gcrnn_fused_seq32s.hip dispatches here when gcrnn_seq32r_lds says there is room)
template <int K, int XS, bool R1>
static int seq32r_launch_rt(const Seq32Args& sa, int rt, size_t lds, hipStream_t st) {
  return rt == 3 ? seq32r_launch_v<K, XS, R1, 3>(sa, lds, st) : seq32r_launch_v<K, XS, R1, 2>(sa, lds, st);
}

int gcrnn_seq32r_forward(const Seq32Args& sa, int K, int XS, int rt, size_t lds, hipStream_t st) {
  if (!sa.a1 || !sa.scr || sa.gi0 || !sa.pk_src0) return GCRNN_ERR_NULL_POINTER;
  if (rt != 2 && rt != 3) return GCRNN_ERR_UNSUPPORTED;
#define GCRNN_SEQ32R_CASE(KK, XX) \
  if (K == KK && XS == XX) { \
    if constexpr (KK == 4 && XX == 2) return sa.r1a ? GCRNN_ERR_UNSUPPORTED : seq32r_launch_rt<KK, XX, false>(sa, rt, lds, st); \
    else return sa.r1a ? seq32r_launch_rt<KK, XX, true>(sa, rt, lds, st) : seq32r_launch_rt<KK, XX, false>(sa, rt, lds, st); \
  }
  GCRNN_SEQ32R_CASE(5, 2) GCRNN_SEQ32R_CASE(4, 2) GCRNN_SEQ32R_CASE(3, 2) GCRNN_SEQ32R_CASE(2, 2)
  GCRNN_SEQ32R_CASE(5, 1) GCRNN_SEQ32R_CASE(4, 1) GCRNN_SEQ32R_CASE(3, 1) GCRNN_SEQ32R_CASE(2, 1)
#undef GCRNN_SEQ32R_CASE
  return GCRNN_ERR_UNSUPPORTED;
}
