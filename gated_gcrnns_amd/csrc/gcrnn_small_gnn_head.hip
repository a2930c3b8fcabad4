// Backward of the one-layer graph-filter head that the small-graph forward evaluates on every state (FWD_GNN of gcrnn_small_mfma.hip):
//   y = act(b + sum_k sum_f w[k][f] (h S^k)[f][n])   =>   dz = dy . act'(y),   dU_0 = dz,   dU_k = dU_{k-1} S^T   (dU_k[m] = sum_n dU_{k-1}[n] S[m][n]).
// With dU [items][K_o][N] the head's share of the state gradient is dH[f][n] = sum_k w[k][f] dU_k[n] -- a per-node head of O = K_o outputs
// fed dY := dU, which the BPTT launch forms itself (gcrnn_small_dense_backward_node_head) -- and d w[k][f] = sum_n dU_k[n] h[f][n],
// d b = sum_n dU_0[n] are gcrnn_node_linear_backward's sums on the same dU. No dH [items][F][N] exists.
// One wave per item, four items per workgroup round; S sits transposed in LDS so that the lanes of a wave read consecutive words.
// Every sum runs over n ascending in one accumulator; no atomics; every element of dU is written.
#include "gcrnn_common.h"
#include "gcrnn_small_mfma.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void gnn_head_adjoint_kernel(const T* __restrict__ dY,     // [items][N]
                                                               const T* __restrict__ Y,      // [items][N]
                                                               const T* __restrict__ Sd,     // [N][N]
                                                               T* __restrict__ dU,           // [items][Ko][N]
                                                               int64_t items, int N, int Ko, int act) {
  extern __shared__ __attribute__((aligned(16))) char smem_gnn_adj[];
  T* St = reinterpret_cast<T*>(smem_gnn_adj);      // [N][N]  St[n][m] = S[m][n]
  T* vb = St + (size_t)N * N;                      // [4 waves][2][N]  level k - 1 | level k of the wave's item
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < N * N; i += 256) {
    const int m = i / N, n = i - m * N;
    St[n * N + m] = Sd[i];
  }
  __syncthreads();
  for (int64_t it0 = (int64_t)blockIdx.x * 4; it0 < items; it0 += (int64_t)gridDim.x * 4) {      // uniform over the workgroup: every wave meets every barrier
    const int64_t it = it0 + wave;
    const bool live = it < items;
    T* v0 = vb + wave * 2 * N;
    T* v1 = v0 + N;
    if (live)
      for (int n = lane; n < N; n += 64) {
        const T d = dY[it * N + n] * gnn_act_grad<T>(Y[it * N + n], act);
        v0[n] = d;
        dU[it * Ko * N + n] = d;
      }
    __syncthreads();
    for (int k = 1; k < Ko; ++k) {
      if (live)
        for (int m = lane; m < N; m += 64) {
          T s = T(0);
#pragma unroll 4
          for (int n = 0; n < N; ++n) s += v0[n] * St[n * N + m];
          v1[m] = s;
          dU[(it * Ko + k) * N + m] = s;
        }
      __syncthreads();
      T* tmp = v0; v0 = v1; v1 = tmp;
    }
  }
}

template <typename T>
int gnn_adjoint_launch(const void* dY, const void* Y, const void* Sd, void* dU, int64_t items, int64_t N, int64_t Ko, int act, hipStream_t st) {
  const size_t lds = gnn_adjoint_lds<T>(N);
  auto kern = gnn_head_adjoint_kernel<T>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  const int64_t rounds = cdiv(items, 4);
  const unsigned grid = (unsigned)(rounds < 1024 ? rounds : 1024);
  GCRNN_PRE_LAUNCH();
  kern<<<grid, 256, lds, st>>>((const T*)dY, (const T*)Y, (const T*)Sd, (T*)dU, items, (int)N, (int)Ko, act);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

}  // namespace

extern "C" int gcrnn_small_gnn_head_adjoint(int dtype, const void* dY, const void* Y, const void* Sdense, void* dU, int64_t items,
                                            int64_t N, int64_t Ko, int act, void* stream) {
  if (!dY || !Y || !Sdense || !dU) return GCRNN_ERR_NULL_POINTER;
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return GCRNN_ERR_BAD_DTYPE;
  if (items <= 0 || N <= 0 || Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT || act < 0 || act > 3) return GCRNN_ERR_BAD_SHAPE;
  if (N > 256 || (dtype == GCRNN_F32 ? gnn_adjoint_lds<float>(N) : gnn_adjoint_lds<double>(N)) > (size_t)160 * 1024) return GCRNN_ERR_UNSUPPORTED;
  return dtype == GCRNN_F32 ? gnn_adjoint_launch<float>(dY, Y, Sdense, dU, items, N, Ko, act, as_stream(stream))
                            : gnn_adjoint_launch<double>(dY, Y, Sdense, dU, items, N, Ko, act, as_stream(stream));
}
