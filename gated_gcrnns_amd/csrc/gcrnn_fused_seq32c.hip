// Instantiations, seed and launcher of the wide BPTT chain with a RANK-1 upstream gradient (gcrnn_fused_seq32.h, MODE 2 with VAR bit 4):
// training of cell + output head Linear(F -> 1) shared by all nodes (the regression model's `multipMlp` head with one output). The loss
// reaches the states as dH_t[f][n] = w_head[f] dy_t[n]; the chain makes that operand in its epilogue from dy [B][T][N] (user layout) and the
// F weights, so neither dH nor its sequence-major copy exists. A translation unit of its own, compiled beside the others.
#include "gcrnn_fused_step.h"
#define GCRNN_SEQ32_STAMP_READER_NAME gcrnn_debug_read_seq32c_stamps      // (diagnostic builds: this unit's own stamp array and reader)
#include "gcrnn_fused_seq32.h"

// dpre[T-1] = bf16(w dy) (1 - h^2): the seed of the chain (t = T-1) on the sequence-major state h [B][NP][F] bf16; dy = dy[0][T-1] in the
// user layout (bstride elements between sequences). One thread per feature pair; rows >= N get dy = 0.
__global__ void seq32_seed_head_kernel(const uint16_t* __restrict__ dy, int64_t bstride, const float* __restrict__ w, const uint16_t* __restrict__ h,
                                       uint16_t* __restrict__ out, int64_t n, int F, int N) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (i >= n) return;
  const int f = (int)(i % F);
  const int64_t row = i / F;
  const int node = (int)(row % NP);
  const int64_t b = row / NP;
  const float dyv = node < N ? bf2f(dy[b * bstride + node]) : 0.f;
  const uint32_t hv = *reinterpret_cast<const uint32_t*>(h + i);
  const float g0 = bf2f(f2bf(w[f] * dyv)), g1 = bf2f(f2bf(w[f + 1] * dyv));
  const float h0 = bf2f((uint16_t)(hv & 0xffffu)), h1 = bf2f((uint16_t)(hv >> 16));
  *reinterpret_cast<uint32_t*>(out + i) = pack2bf(g0 * (1.f - h0 * h0), g1 * (1.f - h1 * h1));
}

int gcrnn_seq32c_seed(const uint16_t* dy, int64_t bstride, const float* w, const uint16_t* h, uint16_t* out, int64_t B, int F, int N, hipStream_t st) {
  const int64_t n = B * NP * F;
  GCRNN_PRE_LAUNCH();
  seq32_seed_head_kernel<<<(unsigned)cdiv(n / 2, 256), 256, 0, st>>>(dy, bstride, w, h, out, n, F, N);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <int K, int HS>
static int seq32c_launch(const Seq32Args& sa, size_t lds, hipStream_t st) {
  auto sk = fused_seq32_kernel<K, HS, 0, 16, 2>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(sk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  sk<<<(unsigned)(sa.B < gcrnn_persistent_grid() ? sa.B : gcrnn_persistent_grid()), STHREADS, lds, st>>>(sa);      // one workgroup per CU
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// the persistent chain with the rank-1 upstream gradient (gcrnn_fused_seq32.hip, gcrnn_fused_backward_data_wide_head_bf16, dispatches here)
int gcrnn_seq32c_chain(const Seq32Args& sa, int K, int HS, hipStream_t st) {
  if (!sa.head_w || sa.r1a || sa.pk_src0) return GCRNN_ERR_UNSUPPORTED;
#define GCRNN_SEQ32C_CASE(KK, HH) \
  if (K == KK && HS == HH) { const size_t lds = Seq32Map<KK, HH, 0>::lds_bytes(sa.entries, false); return lds ? seq32c_launch<KK, HH>(sa, lds, st) : GCRNN_ERR_UNSUPPORTED; }
  GCRNN_SEQ32C_CASE(5, 2) GCRNN_SEQ32C_CASE(4, 2) GCRNN_SEQ32C_CASE(3, 2) GCRNN_SEQ32C_CASE(2, 2)
  GCRNN_SEQ32C_CASE(5, 1) GCRNN_SEQ32C_CASE(4, 1) GCRNN_SEQ32C_CASE(3, 1) GCRNN_SEQ32C_CASE(2, 1)
#undef GCRNN_SEQ32C_CASE
  return GCRNN_ERR_UNSUPPORTED;
}
