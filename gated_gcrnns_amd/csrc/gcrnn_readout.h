// LDS layout of the graph-filter layer kernels (gcrnn_readout.hip), shared with the host-side queries (gcrnn_host.cpp) so that the
// `supported` answer and the launch agree byte for byte.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define GFL_HD __host__ __device__
#else
#define GFL_HD
#endif

constexpr int64_t GFL_MAX_N = 1024;            // node rows: col indices live in LDS as uint16
constexpr int64_t GFL_LDS_BYTES = 160 * 1024;  // one workgroup may use the whole CU's LDS
constexpr int64_t GFL_CUS = 256;               // slot count is a function of the shape alone (deterministic on every device)

struct GflLayout {
  int64_t w, b, dw, db, rowptr, col, val, sig, total;
};

static inline GFL_HD int64_t gfl_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// Forward: w [K*F_out][F_in], b [F_out], CSR(S^T), signals: K*F_out rows (taps first, F_out < F_in) or K*F_in rows (hops first).
// Backward: w, dW accumulator [K*F_out][F_in], db accumulator [F_out], CSR(S), signals u_k: K*F_out rows.
// acc = 4 (bf16 / fp32 data) or 8 (fp64); uniform != 0: every edge has one weight, the value array is not kept.
static inline GFL_HD GflLayout gfl_layout(int64_t N, int64_t nnz, int64_t Fin, int64_t Fout, int64_t K, int64_t acc, int backward,
                                          int uniform) {
  GflLayout L;
  const int64_t KO = K * Fout;
  int64_t off = 0;
  L.w = off;      off = gfl_align16(off + KO * Fin * acc);
  L.b = off;      off = gfl_align16(off + Fout * acc);
  L.dw = off;     off = gfl_align16(off + (backward ? KO * Fin * acc : 0));
  L.db = off;     off = gfl_align16(off + (backward ? Fout * acc : 0));
  L.rowptr = off; off = gfl_align16(off + (N + 1) * 4);
  L.col = off;    off = gfl_align16(off + nnz * 2);
  L.val = off;    off = gfl_align16(off + (uniform ? 0 : nnz * acc));
  L.sig = off;    off = gfl_align16(off + K * ((backward || Fout < Fin) ? Fout : Fin) * N * acc);
  L.total = off;
  return L;
}
