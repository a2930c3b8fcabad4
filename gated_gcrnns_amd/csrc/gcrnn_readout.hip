// One graph-filter layer with bias and activation: the GNN output heads (SelectionGNN layers, architectures.py:10-177, and the
// Selection-GNN C(S) of the gated GCRNNs) on the user layout, one launch per pass, no intermediate tensor in HBM.
//   forward   y[i][o][n] = act( sum_k sum_f w[o][0][k][f] (x_i S^k)[f][n] + b[o] ),   (x S)[f][n] = sum_m x[f][m] S[m][n]
//   backward  g = dy * act'(y) (from the stored y),  u_k = g (S^T)^k  (K-1 hops on F_out channels),
//             dx[f][n] = sum_{o,k} w[o][k][f] u_k[o][n],   dW[o][k][f] = sum_{i,n} x[f][n] u_k[o][n],   db[o] = sum_{i,n} g[o][n]
// x [items][F_in][N] (bf16, fp32 or fp64), w [F_out][1][K][F_in], b [F_out], y / dy [items][F_out][N] in the accumulation type
// (fp32 for bf16 / fp32 data, fp64 for fp64), dx in x's type. Each workgroup walks items blockIdx.x, + gridDim.x, ... with the CSR
// rows, the weights and the running signals in LDS:
//   taps first (F_out < F_in): s_k = C_k x in registers while x streams by once, then Horner acc <- acc S + s_k on F_out channels
//     (the node gates' F -> 1 filter does the same, gcrnn_node_gate.hip), bias + activation in the last hop's epilogue;
//   hops first (F_out >= F_in): z_k = z_{k-1} S on F_in channels, then y = sum_k C_k z_k.
// The weight / bias gradients are per-workgroup partial sums (one slot per workgroup, fixed item order, no atomics) that the
// caller adds in a fixed order: two runs give the same bits.
#include "gcrnn_common.h"
#include "gcrnn_readout.h"

namespace {

constexpr int GFL_THREADS = 256, GFL_WAVES = GFL_THREADS / 64, GFL_J = 8;

__device__ __forceinline__ float gfl_bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint16_t gfl_f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

template <typename T, typename A> __device__ __forceinline__ A gfl_cvt(T v) {
  if constexpr (sizeof(T) == 2) return gfl_bf2f(v); else return (A)v;
}
template <typename T, typename A> __device__ __forceinline__ T gfl_out(A v) {
  if constexpr (sizeof(T) == 2) return gfl_f2bf(v); else return (T)v;
}

// VEC consecutive elements of a node-contiguous row (VEC = 4: 8-byte bf16 / 16-byte fp32 vectors)
template <typename T, typename A, int VEC> __device__ __forceinline__ void gfl_load(const T* p, A (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = gfl_cvt<T, A>(p[0]);
  } else if constexpr (sizeof(T) == 2) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] = gfl_bf2f((uint16_t)(u.x & 0xffffu)); v[1] = gfl_bf2f((uint16_t)(u.x >> 16));
    v[2] = gfl_bf2f((uint16_t)(u.y & 0xffffu)); v[3] = gfl_bf2f((uint16_t)(u.y >> 16));
  } else {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
}
template <typename T, typename A, int VEC> __device__ __forceinline__ void gfl_store(T* p, const A (&v)[VEC]) {
  if constexpr (VEC == 1) {
    p[0] = gfl_out<T, A>(v[0]);
  } else if constexpr (sizeof(T) == 2) {
    uint2 u;
    u.x = (uint32_t)gfl_f2bf(v[0]) | ((uint32_t)gfl_f2bf(v[1]) << 16);
    u.y = (uint32_t)gfl_f2bf(v[2]) | ((uint32_t)gfl_f2bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = u;
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// act: 0 identity, 1 ReLU, 2 tanh, 3 sigmoid; the derivative is taken from the activation's OUTPUT
template <typename A> __device__ __forceinline__ A gfl_act(A v, int act) {
  if (act == 1) return v <= A(0) ? A(0) : v;      // (as torch.relu: a NaN stays a NaN)
  if (act == 2) return tanh(v);
  if (act == 3) return A(1) / (A(1) + exp(-v));
  return v;
}
template <typename A> __device__ __forceinline__ A gfl_act_grad(A y, int act) {
  if (act == 1) return y > A(0) ? A(1) : A(0);
  if (act == 2) return A(1) - y * y;
  if (act == 3) return y * (A(1) - y);
  return A(1);
}

template <typename A> __device__ __forceinline__ A gfl_wave_sum(A v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  return v;
}

// one row of the shift: sum_{e in row n} val[e] src[col[e]]  (uniform: every edge weighs uw, no value array)
template <typename A>
__device__ __forceinline__ A gfl_hop(const A* src, const int32_t* rp, const uint16_t* cl, const A* vl, bool uniform, A uw, int n) {
  const int e0 = rp[n], e1 = rp[n + 1];
  A s = A(0);
  if (uniform) {
    for (int e = e0; e < e1; ++e) s += src[cl[e]];
    return s * uw;
  }
  for (int e = e0; e < e1; ++e) s += vl[e] * src[cl[e]];
  return s;
}

template <typename A>
__device__ void gfl_stage_graph(unsigned char* smem, const GflLayout& L, const int32_t* rowptr, const int32_t* col, const A* val,
                                int N, int nnz, bool uniform) {
  int32_t* rp = (int32_t*)(smem + L.rowptr);
  uint16_t* cl = (uint16_t*)(smem + L.col);
  A* vl = (A*)(smem + L.val);
  for (int i = threadIdx.x; i <= N; i += GFL_THREADS) rp[i] = rowptr[i];
  for (int i = threadIdx.x; i < nnz; i += GFL_THREADS) {
    cl[i] = (uint16_t)col[i];
    if (!uniform) vl[i] = val[i];
  }
}

template <typename T, typename A, int VEC>
__global__ __launch_bounds__(GFL_THREADS) void gfl_forward_kernel(const T* __restrict__ x, const A* __restrict__ w, const A* __restrict__ b,
                                                                   A* __restrict__ y, const int32_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ col, const A* __restrict__ val, int uniform,
                                                                   A uw, int64_t items, int N, int nnz, int Fin, int Fout, int K, int act) {
  extern __shared__ __align__(16) unsigned char smem[];
  const GflLayout L = gfl_layout(N, nnz, Fin, Fout, K, sizeof(A), 0, uniform);
  A* ws = (A*)(smem + L.w);
  A* bs = (A*)(smem + L.b);
  const int32_t* rp = (const int32_t*)(smem + L.rowptr);
  const uint16_t* cl = (const uint16_t*)(smem + L.col);
  const A* vl = (const A*)(smem + L.val);
  A* sig = (A*)(smem + L.sig);
  const int KO = K * Fout, tid = threadIdx.x;
  for (int i = tid; i < KO * Fin; i += GFL_THREADS) ws[i] = w[i];          // [F_out][1][K][F_in] = row j = o K + k of C
  for (int i = tid; i < Fout; i += GFL_THREADS) bs[i] = b ? b[i] : A(0);
  gfl_stage_graph<A>(smem, L, rowptr, col, val, N, nnz, uniform != 0);
  __syncthreads();
  const bool taps_first = Fout < Fin;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const T* xi = x + it * Fin * N;
    A* yi = y + it * Fout * N;
    if (taps_first) {
      // s_j[n] = sum_f C[j][f] x[f][n], j = o K + k: x read once (per chunk of GFL_J rows of C), coalesced over n
      for (int jc = 0; jc < KO; jc += GFL_J) {
        for (int n0 = tid * VEC; n0 < N; n0 += GFL_THREADS * VEC) {
          A acc[GFL_J][VEC];
#pragma unroll
          for (int q = 0; q < GFL_J; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[q][v] = A(0);
#pragma unroll 4
          for (int f = 0; f < Fin; ++f) {
            A xv[VEC];
            gfl_load<T, A, VEC>(xi + (int64_t)f * N + n0, xv);
#pragma unroll
            for (int q = 0; q < GFL_J; ++q) {
              if (jc + q < KO) {
                const A wq = ws[(jc + q) * Fin + f];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[q][v] += wq * xv[v];
              }
            }
          }
#pragma unroll
          for (int q = 0; q < GFL_J; ++q)
            if (jc + q < KO)
#pragma unroll
              for (int v = 0; v < VEC; ++v) sig[(jc + q) * N + n0 + v] = acc[q][v];
        }
      }
      __syncthreads();
      if (K == 1) {
        for (int e = tid; e < Fout * N; e += GFL_THREADS) {
          const int o = e / N;
          yi[e] = gfl_act(sig[e] + bs[o], act);
        }
      }
      // Horner: acc_k = acc_{k+1} S + s_k, written over s_k; the last hop adds the bias, activates and stores y
      for (int k = K - 2; k >= 0; --k) {
        for (int e = tid; e < Fout * N; e += GFL_THREADS) {
          const int o = e / N, n = e - o * N;
          const A v = sig[(o * K + k) * N + n] + gfl_hop(sig + (o * K + k + 1) * N, rp, cl, vl, uniform != 0, uw, n);
          if (k > 0) sig[(o * K + k) * N + n] = v;
          else yi[e] = gfl_act(v + bs[o], act);
        }
        __syncthreads();
      }
      if (K == 1) __syncthreads();
    } else {
      // z_0 = x, z_k = z_{k-1} S on F_in channels (signal rows k F_in + f), then y = sum_k C_k z_k
      for (int e = tid; e < Fin * N; e += GFL_THREADS) sig[e] = gfl_cvt<T, A>(xi[e]);
      __syncthreads();
      for (int k = 1; k < K; ++k) {
        for (int e = tid; e < Fin * N; e += GFL_THREADS) {
          const int f = e / N, n = e - f * N;
          sig[(k * Fin + f) * N + n] = gfl_hop(sig + ((k - 1) * Fin + f) * N, rp, cl, vl, uniform != 0, uw, n);
        }
        __syncthreads();
      }
      for (int e = tid; e < Fout * N; e += GFL_THREADS) {
        const int o = e / N, n = e - o * N;
        A a = bs[o];
        for (int k = 0; k < K; ++k)
          for (int f = 0; f < Fin; ++f) a += ws[(o * K + k) * Fin + f] * sig[(k * Fin + f) * N + n];
        yi[e] = gfl_act(a, act);
      }
      __syncthreads();
    }
  }
}

template <typename T, typename A, int VEC>
__global__ __launch_bounds__(GFL_THREADS) void gfl_backward_kernel(const T* __restrict__ x, const A* __restrict__ w, const A* __restrict__ y,
                                                                    const A* __restrict__ dy, T* __restrict__ dx, A* __restrict__ dw_parts,
                                                                    A* __restrict__ db_parts, const int32_t* __restrict__ rowptr,
                                                                    const int32_t* __restrict__ col, const A* __restrict__ val, int uniform,
                                                                    A uw, int64_t items, int N, int nnz, int Fin, int Fout, int K, int act) {
  extern __shared__ __align__(16) unsigned char smem[];
  const GflLayout L = gfl_layout(N, nnz, Fin, Fout, K, sizeof(A), 1, uniform);
  A* ws = (A*)(smem + L.w);
  A* dws = (A*)(smem + L.dw);
  A* dbs = (A*)(smem + L.db);
  const int32_t* rp = (const int32_t*)(smem + L.rowptr);
  const uint16_t* cl = (const uint16_t*)(smem + L.col);
  const A* vl = (const A*)(smem + L.val);
  A* sig = (A*)(smem + L.sig);                      // u_k of channel o at row j = o K + k (the row of C it meets)
  const int KO = K * Fout, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < KO * Fin; i += GFL_THREADS) { ws[i] = w[i]; dws[i] = A(0); }
  for (int i = tid; i < Fout; i += GFL_THREADS) dbs[i] = A(0);
  gfl_stage_graph<A>(smem, L, rowptr, col, val, N, nnz, uniform != 0);
  __syncthreads();
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const T* xi = x + it * Fin * N;
    T* dxi = dx ? dx + it * Fin * N : nullptr;
    for (int e = tid; e < Fout * N; e += GFL_THREADS) {
      const int o = e / N, n = e - o * N;
      sig[o * K * N + n] = dy[it * Fout * N + e] * gfl_act_grad(y[it * Fout * N + e], act);
    }
    __syncthreads();
    for (int o = wave; o < Fout; o += GFL_WAVES) {          // db: one wave per channel, fixed order
      A s = A(0);
      for (int n = lane; n < N; n += 64) s += sig[o * K * N + n];
      s = gfl_wave_sum(s);
      if (lane == 0) dbs[o] += s;
    }
    for (int k = 1; k < K; ++k) {                           // u_k = u_{k-1} S^T: rows of CSR(S)
      for (int e = tid; e < Fout * N; e += GFL_THREADS) {
        const int o = e / N, n = e - o * N;
        sig[(o * K + k) * N + n] = gfl_hop(sig + (o * K + k - 1) * N, rp, cl, vl, uniform != 0, uw, n);
      }
      __syncthreads();
    }
    // dx and dW, one wave per input channel f (fixed owner: the dW accumulator row needs no barrier)
    for (int f = wave; f < Fin; f += GFL_WAVES) {
      const T* xr = xi + (int64_t)f * N;
      T* dxr = dxi ? dxi + (int64_t)f * N : nullptr;
      if (KO <= GFL_J) {
        A wf[GFL_J], p[GFL_J];
#pragma unroll
        for (int q = 0; q < GFL_J; ++q) { wf[q] = q < KO ? ws[q * Fin + f] : A(0); p[q] = A(0); }
#pragma unroll 4
        for (int n0 = lane * VEC; n0 < N; n0 += 64 * VEC) {
          A xv[VEC], d[VEC];
          gfl_load<T, A, VEC>(xr + n0, xv);
#pragma unroll
          for (int v = 0; v < VEC; ++v) d[v] = A(0);
#pragma unroll
          for (int q = 0; q < GFL_J; ++q) {
            if (q < KO) {
#pragma unroll
              for (int v = 0; v < VEC; ++v) {
                const A uv = sig[q * N + n0 + v];
                d[v] += wf[q] * uv;
                p[q] += xv[v] * uv;
              }
            }
          }
          if (dxr) gfl_store<T, A, VEC>(dxr + n0, d);
        }
#pragma unroll
        for (int q = 0; q < GFL_J; ++q) {
          if (q < KO) {
            const A s = gfl_wave_sum(p[q]);
            if (lane == 0) dws[q * Fin + f] += s;
          }
        }
      } else {
        if (dxr) {
          for (int n0 = lane * VEC; n0 < N; n0 += 64 * VEC) {
            A d[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) d[v] = A(0);
            for (int j = 0; j < KO; ++j) {
              const A wj = ws[j * Fin + f];
#pragma unroll
              for (int v = 0; v < VEC; ++v) d[v] += wj * sig[j * N + n0 + v];
            }
            gfl_store<T, A, VEC>(dxr + n0, d);
          }
        }
        for (int jc = 0; jc < KO; jc += GFL_J) {
          A p[GFL_J];
#pragma unroll
          for (int q = 0; q < GFL_J; ++q) p[q] = A(0);
          for (int n0 = lane * VEC; n0 < N; n0 += 64 * VEC) {
            A xv[VEC];
            gfl_load<T, A, VEC>(xr + n0, xv);
#pragma unroll
            for (int q = 0; q < GFL_J; ++q)
              if (jc + q < KO)
#pragma unroll
                for (int v = 0; v < VEC; ++v) p[q] += xv[v] * sig[(jc + q) * N + n0 + v];
          }
#pragma unroll
          for (int q = 0; q < GFL_J; ++q) {
            if (jc + q < KO) {
              const A s = gfl_wave_sum(p[q]);
              if (lane == 0) dws[(jc + q) * Fin + f] += s;
            }
          }
        }
      }
    }
    __syncthreads();                                          // sig is rewritten by the next item
  }
  for (int i = tid; i < KO * Fin; i += GFL_THREADS) dw_parts[(int64_t)blockIdx.x * KO * Fin + i] = dws[i];
  if (db_parts)
    for (int i = tid; i < Fout; i += GFL_THREADS) db_parts[(int64_t)blockIdx.x * Fout + i] = dbs[i];
}

struct GflArgs {
  int64_t items, N, nnz, Fin, Fout, K;
  int act;
};

template <typename T, typename A, int VEC>
int gfl_launch_forward(const void* x, const void* w, const void* b, void* y, const int32_t* rowptr, const int32_t* col, const void* val,
                       double uw, const GflArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  auto kern = gfl_forward_kernel<T, A, VEC>;
  const int uniform = uw != 0.0;      // the flag the host sized LDS with, not a re-test of the value after its cast to A
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kern<<<(unsigned)grid, GFL_THREADS, lds, st>>>((const T*)x, (const A*)w, (const A*)b, (A*)y, rowptr, col, (const A*)val, uniform, (A)uw, a.items,
                                                 (int)a.N, (int)a.nnz, (int)a.Fin, (int)a.Fout, (int)a.K, a.act);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <typename T, typename A, int VEC>
int gfl_launch_backward(const void* x, const void* w, const void* y, const void* dy, void* dx, void* dwp, void* dbp, const int32_t* rowptr,
                        const int32_t* col, const void* val, double uw, const GflArgs& a, int64_t grid, size_t lds, hipStream_t st) {
  auto kern = gfl_backward_kernel<T, A, VEC>;
  const int uniform = uw != 0.0;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kern<<<(unsigned)grid, GFL_THREADS, lds, st>>>((const T*)x, (const A*)w, (const A*)y, (const A*)dy, (T*)dx, (A*)dwp, (A*)dbp, rowptr, col,
                                                 (const A*)val, uniform, (A)uw, a.items, (int)a.N, (int)a.nnz, (int)a.Fin, (int)a.Fout, (int)a.K, a.act);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// argument checks shared by both passes; VEC = 4 where rows are whole 4-element vectors on aligned storage
int gfl_check(int dtype, const void* x, const void* w, const void* out, const int32_t* rowptr, const int32_t* col, const void* val,
              double uw, const GflArgs& a, int64_t E) {
  if (!x || !w || !out || !rowptr || (a.nnz > 0 && !col) || (a.nnz > 0 && uw == 0.0 && !val)) return GCRNN_ERR_NULL_POINTER;
  if (a.items <= 0 || a.N <= 0 || a.nnz < 0 || a.Fin <= 0 || a.Fout <= 0 || a.K <= 0 || a.act < 0 || a.act > 3) return GCRNN_ERR_BAD_SHAPE;
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64 && dtype != GCRNN_BF16) return GCRNN_ERR_BAD_DTYPE;
  if (!gcrnn_graph_filter_layer_supported(dtype, a.N, a.nnz, E, a.Fin, a.Fout, a.K, uw != 0.0)) return GCRNN_ERR_UNSUPPORTED;
  return GCRNN_OK;
}

bool gfl_vec4(int dtype, int64_t N, const void* p0, const void* p1) {
  const uintptr_t al = dtype == GCRNN_BF16 ? 8 : 16;
  return dtype != GCRNN_F64 && N % 4 == 0 && (uintptr_t)p0 % al == 0 && (p1 == nullptr || (uintptr_t)p1 % al == 0);
}

}  // namespace

extern "C" int gcrnn_graph_filter_layer_forward(int dtype, const void* x, const void* w, const void* b, void* y, const int32_t* rowptr,
                                                const int32_t* col, const void* val, double uniform_w, int64_t items, int64_t N,
                                                int64_t nnz, int64_t E, int64_t F_in, int64_t F_out, int64_t K, int act, void* stream) {
  const GflArgs a{items, N, nnz, F_in, F_out, K, act};
  const int st = gfl_check(dtype, x, w, y, rowptr, col, val, uniform_w, a, E);
  if (st != GCRNN_OK) return st;
  const int acc = dtype == GCRNN_F64 ? 8 : 4;
  const size_t lds = (size_t)gfl_layout(N, nnz, F_in, F_out, K, acc, 0, uniform_w != 0.0).total;
  const int64_t grid = gcrnn_graph_filter_layer_wgrad_slots(dtype, items, N, nnz, F_in, F_out, K, uniform_w != 0.0);
  const bool v4 = gfl_vec4(dtype, N, x, nullptr);
  hipStream_t s = as_stream(stream);
  if (dtype == GCRNN_BF16)
    return v4 ? gfl_launch_forward<uint16_t, float, 4>(x, w, b, y, rowptr, col, val, uniform_w, a, grid, lds, s)
              : gfl_launch_forward<uint16_t, float, 1>(x, w, b, y, rowptr, col, val, uniform_w, a, grid, lds, s);
  if (dtype == GCRNN_F32)
    return v4 ? gfl_launch_forward<float, float, 4>(x, w, b, y, rowptr, col, val, uniform_w, a, grid, lds, s)
              : gfl_launch_forward<float, float, 1>(x, w, b, y, rowptr, col, val, uniform_w, a, grid, lds, s);
  return gfl_launch_forward<double, double, 1>(x, w, b, y, rowptr, col, val, uniform_w, a, grid, lds, s);
}

extern "C" int gcrnn_graph_filter_layer_backward(int dtype, const void* x, const void* w, const void* y, const void* dy, void* dx,
                                                 void* dw_parts, void* db_parts, int64_t slots, const int32_t* rowptr, const int32_t* col,
                                                 const void* val, double uniform_w, int64_t items, int64_t N, int64_t nnz, int64_t E,
                                                 int64_t F_in, int64_t F_out, int64_t K, int act, void* stream) {
  const GflArgs a{items, N, nnz, F_in, F_out, K, act};
  int st = gfl_check(dtype, x, w, dw_parts, rowptr, col, val, uniform_w, a, E);
  if (st != GCRNN_OK) return st;
  if (!y || !dy) return GCRNN_ERR_NULL_POINTER;
  const int64_t grid = gcrnn_graph_filter_layer_wgrad_slots(dtype, items, N, nnz, F_in, F_out, K, uniform_w != 0.0);
  if (slots != grid) return GCRNN_ERR_WORKSPACE;
  const int acc = dtype == GCRNN_F64 ? 8 : 4;
  const size_t lds = (size_t)gfl_layout(N, nnz, F_in, F_out, K, acc, 1, uniform_w != 0.0).total;
  const bool v4 = gfl_vec4(dtype, N, x, dx);
  hipStream_t s = as_stream(stream);
  if (dtype == GCRNN_BF16)
    return v4 ? gfl_launch_backward<uint16_t, float, 4>(x, w, y, dy, dx, dw_parts, db_parts, rowptr, col, val, uniform_w, a, grid, lds, s)
              : gfl_launch_backward<uint16_t, float, 1>(x, w, y, dy, dx, dw_parts, db_parts, rowptr, col, val, uniform_w, a, grid, lds, s);
  if (dtype == GCRNN_F32)
    return v4 ? gfl_launch_backward<float, float, 4>(x, w, y, dy, dx, dw_parts, db_parts, rowptr, col, val, uniform_w, a, grid, lds, s)
              : gfl_launch_backward<float, float, 1>(x, w, y, dy, dx, dw_parts, db_parts, rowptr, col, val, uniform_w, a, grid, lds, s);
  return gfl_launch_backward<double, double, 1>(x, w, y, dy, dx, dw_parts, db_parts, rowptr, col, val, uniform_w, a, grid, lds, s);
}
