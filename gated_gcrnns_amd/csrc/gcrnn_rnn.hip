// The drivers' plain-RNN baseline (reference RNNforRegression / RNNforClassification = torch.nn.RNN, one layer, batch_first):
//   h_t = act( W_ih x_t + b_ih + W_hh h_{t-1} + b_hh ),  act = tanh or ReLU,  x [B][T][D], h0 [B][F_h], H [B][T][F_h].
// forward   (2 launches)  U = X W_ih^T + b_ih + b_hh  written into H (rnn_gemm_kernel, parallel over the B*T rows), then the
//                         recurrence (rnn_forward_kernel): one 64-lane workgroup per sequence, lane j owns unit j with row j of
//                         W_hh in registers, h_{t-1} broadcast through a double-buffered LDS vector, all T steps in one launch;
//                         each step reads U[b][t] from H and overwrites it with h_t (H is the only output).
// backward  (<= 3 launches) BPTT (rnn_bptt_kernel), the same shape with column j of W_hh in lane j:
//                         dz_t = (dH_t + W_hh^T dz_{t+1}) * act'(h_t), act' from h_t alone (1 - h^2, h > 0); dh0 = W_hh^T dz_0;
//                         the weight gradients (rnn_wgrad_kernel) of [W_ih | W_hh | b] = sum_rows dz_r [x_r | h_{r-1} | 1]^T, as
//                         per-slot partial sums over a fixed range of rows each (no atomics; the caller adds the slots in a
//                         fixed order: two runs give the same bits); dX = dZ W_ih (rnn_gemm_kernel) only when asked for.
// Every launch count is independent of T. fp32 or fp64 throughout.
#include "gcrnn_common.h"
#include "gcrnn_rnn.h"

namespace {

constexpr int RNN_GEMM_THREADS = 256, RNN_GEMM_M = 64, RNN_GEMM_N = 64, RNN_GEMM_K = 16;
constexpr int RNN_WG_THREADS = 256, RNN_WG_ROWS = 32;

template <typename A> __device__ __forceinline__ A rnn_act(A z, int relu) {
  if (relu) return z <= A(0) ? A(0) : z;      // (as torch.relu: a NaN stays a NaN)
  return tanh(z);
}
template <typename A> __device__ __forceinline__ A rnn_act_grad(A h, int relu) {
  if (relu) return h > A(0) ? A(1) : A(0);
  return A(1) - h * h;
}

// C[m][n] = sum_k Am[m*lda + k] * Bm[k*sbk + n*sbn] (+ bias1[n] + bias2[n]), C row stride ldc; 64 x 64 tile per workgroup,
// 4 x 4 outputs per thread, K in chunks of 16 through LDS. Used for U = X W_ih^T (+ biases) and dX = dZ W_ih.
template <typename A>
__global__ __launch_bounds__(RNN_GEMM_THREADS) void rnn_gemm_kernel(const A* __restrict__ Am, const A* __restrict__ Bm,
                                                                     const A* __restrict__ bias1, const A* __restrict__ bias2,
                                                                     A* __restrict__ Cm, int64_t M, int Nc, int K, int64_t lda,
                                                                     int64_t sbk, int64_t sbn, int64_t ldc) {
  __shared__ A As[RNN_GEMM_K][RNN_GEMM_M + 1];
  __shared__ A Bs[RNN_GEMM_K][RNN_GEMM_N + 1];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int64_t m0 = (int64_t)blockIdx.x * RNN_GEMM_M;
  const int n0 = blockIdx.y * RNN_GEMM_N;
  A acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = A(0);
  for (int k0 = 0; k0 < K; k0 += RNN_GEMM_K) {
#pragma unroll
    for (int r = 0; r < (RNN_GEMM_M * RNN_GEMM_K) / RNN_GEMM_THREADS; ++r) {
      const int e = tid + r * RNN_GEMM_THREADS, kk = e % RNN_GEMM_K, mm = e / RNN_GEMM_K;
      const int64_t m = m0 + mm;
      const int k = k0 + kk;
      As[kk][mm] = (m < M && k < K) ? Am[m * lda + k] : A(0);
    }
#pragma unroll
    for (int r = 0; r < (RNN_GEMM_N * RNN_GEMM_K) / RNN_GEMM_THREADS; ++r) {
      const int e = tid + r * RNN_GEMM_THREADS;
      const int kk = sbn == 1 ? e / RNN_GEMM_N : e % RNN_GEMM_K;   // the contiguous index runs fastest across the lanes
      const int nn = sbn == 1 ? e % RNN_GEMM_N : e / RNN_GEMM_K;
      const int n = n0 + nn, k = k0 + kk;
      Bs[kk][nn] = (n < Nc && k < K) ? Bm[(int64_t)k * sbk + (int64_t)n * sbn] : A(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < RNN_GEMM_K; ++kk) {
      A a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = Bs[kk][tx + 16 * q];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] += a[i] * b[q];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + tx + 16 * q;
    if (n >= Nc) continue;
    const A bb = (bias1 ? bias1[n] : A(0)) + (bias2 ? bias2[n] : A(0));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = m0 + ty + 16 * i;
      if (m < M) Cm[m * ldc + n] = acc[i][q] + bb;
    }
  }
}

// One workgroup (one wave) per sequence b. H[b] holds U[b] on entry and h_1..h_T on exit.
template <typename A, int FP>
__global__ __launch_bounds__(64) void rnn_forward_kernel(const A* __restrict__ h0, const A* __restrict__ whh, A* __restrict__ H,
                                                         int T, int Fh, int relu) {
  __shared__ A hs[2][FP];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool own = j < Fh;
  A w[FP];
#pragma unroll
  for (int k = 0; k < FP; ++k) w[k] = (own && k < Fh) ? whh[j * Fh + k] : A(0);
  if (j < FP) hs[1][j] = own ? h0[(int64_t)b * Fh + j] : A(0);      // step 0 reads buffer (0 - 1) & 1
  __syncthreads();
  A* Hb = H + (int64_t)b * T * Fh;
  A u = own ? Hb[j] : A(0);
  for (int t = 0; t < T; ++t) {
    const A un = (own && t + 1 < T) ? Hb[(int64_t)(t + 1) * Fh + j] : A(0);   // next step's input term, ahead of the chain
    const A* hp = hs[(t + 1) & 1];
    A z = u;
#pragma unroll
    for (int k = 0; k < FP; ++k) z += w[k] * hp[k];
    const A h = rnn_act(z, relu);
    if (own) Hb[(int64_t)t * Fh + j] = h;
    if (j < FP) hs[t & 1][j] = own ? h : A(0);
    __syncthreads();      // one wave per workgroup: orders this step's LDS write before the next step's reads
    u = un;
  }
}

// BPTT, one workgroup (one wave) per sequence b: dZ[b][t] for t = T-1 .. 0 and dh0[b] (may be NULL).
template <typename A, int FP>
__global__ __launch_bounds__(64) void rnn_bptt_kernel(const A* __restrict__ whh, const A* __restrict__ H, const A* __restrict__ dH,
                                                      A* __restrict__ dZ, A* __restrict__ dh0, int T, int Fh, int relu) {
  __shared__ A gs[2][FP];
  const int b = blockIdx.x, j = threadIdx.x;
  const bool own = j < Fh;
  A w[FP];                                                          // column j of W_hh: (W_hh^T dz)_j = sum_k W_hh[k][j] dz_k
#pragma unroll
  for (int k = 0; k < FP; ++k) w[k] = (own && k < Fh) ? whh[k * Fh + j] : A(0);
  if (j < FP) gs[1][j] = A(0);                                      // dz_T = 0
  __syncthreads();
  const int64_t base = (int64_t)b * T * Fh;
  A g = own ? dH[base + (int64_t)(T - 1) * Fh + j] : A(0);
  A h = own ? H[base + (int64_t)(T - 1) * Fh + j] : A(0);
  for (int s = 0; s < T; ++s) {
    const int t = T - 1 - s;
    A gn = A(0), hn = A(0);
    if (own && t > 0) {
      gn = dH[base + (int64_t)(t - 1) * Fh + j];
      hn = H[base + (int64_t)(t - 1) * Fh + j];
    }
    const A* zp = gs[(s + 1) & 1];
#pragma unroll
    for (int k = 0; k < FP; ++k) g += w[k] * zp[k];
    const A dz = g * rnn_act_grad(h, relu);
    if (own) dZ[base + (int64_t)t * Fh + j] = dz;
    if (j < FP) gs[s & 1][j] = own ? dz : A(0);
    __syncthreads();
    g = gn;
    h = hn;
  }
  if (dh0 && own) {
    const A* zp = gs[(T - 1) & 1];
    A d = A(0);
#pragma unroll
    for (int k = 0; k < FP; ++k) d += w[k] * zp[k];
    dh0[(int64_t)b * Fh + j] = d;
  }
}

// Weight gradients: parts[slot][j][c] = sum_{rows r of the slot} dZ[r][j] * a_r[c], a_r = [x_r (D) | h_{r-1} (F_h) | 1], with
// h_{r-1} = H[b][t-1] (h0[b] at t = 0). Grid (column tiles, slots); rows of a slot in ascending order: deterministic.
template <typename A, int FP>
__global__ __launch_bounds__(RNN_WG_THREADS) void rnn_wgrad_kernel(const A* __restrict__ X, const A* __restrict__ h0,
                                                                   const A* __restrict__ H, const A* __restrict__ dZ,
                                                                   A* __restrict__ parts, int64_t rows, int64_t rows_per_slot, int T,
                                                                   int D, int Fh) {
  constexpr int JPT = (FP + 3) / 4;                                 // hidden units per thread (4 groups of 64 lanes)
  __shared__ A Zs[RNN_WG_ROWS][FP];
  __shared__ A Xs[RNN_WG_ROWS][RNN_COLS_TILE];
  const int tid = threadIdx.x, cl = tid % RNN_COLS_TILE, jg = tid / RNN_COLS_TILE;
  const int64_t cols = (int64_t)D + Fh + 1;
  const int64_t c = (int64_t)blockIdx.x * RNN_COLS_TILE + cl;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slot;
  const int64_t r1 = r0 + rows_per_slot < rows ? r0 + rows_per_slot : rows;
  A acc[JPT];
#pragma unroll
  for (int i = 0; i < JPT; ++i) acc[i] = A(0);
  for (int64_t rb = r0; rb < r1; rb += RNN_WG_ROWS) {
    for (int e = tid; e < RNN_WG_ROWS * FP; e += RNN_WG_THREADS) {
      const int rr = e / FP, jj = e % FP;
      const int64_t r = rb + rr;
      Zs[rr][jj] = (r < r1 && jj < Fh) ? dZ[r * Fh + jj] : A(0);
    }
    for (int rr = jg; rr < RNN_WG_ROWS; rr += RNN_WG_THREADS / RNN_COLS_TILE) {
      const int64_t r = rb + rr;
      A v = A(0);
      if (r < r1 && c < cols) {
        if (c < D) {
          v = X[r * D + c];
        } else if (c < (int64_t)D + Fh) {
          const int64_t t = r % T;
          v = t > 0 ? H[(r - 1) * Fh + (c - D)] : h0[(r / T) * Fh + (c - D)];
        } else {
          v = A(1);
        }
      }
      Xs[rr][cl] = v;
    }
    __syncthreads();
    for (int rr = 0; rr < RNN_WG_ROWS; ++rr) {
      const A xv = Xs[rr][cl];
#pragma unroll
      for (int i = 0; i < JPT; ++i) {
        const int jj = jg + 4 * i;
        if (jj < FP) acc[i] += Zs[rr][jj] * xv;
      }
    }
    __syncthreads();
  }
  if (c >= cols) return;
  A* out = parts + (int64_t)blockIdx.y * Fh * cols;
#pragma unroll
  for (int i = 0; i < JPT; ++i) {
    const int jj = jg + 4 * i;
    if (jj < Fh) out[(int64_t)jj * cols + c] = acc[i];
  }
}

template <typename A>
int rnn_gemm(const A* Am, const A* Bm, const A* b1, const A* b2, A* Cm, int64_t M, int64_t Nc, int64_t K, int64_t lda, int64_t sbk,
             int64_t sbn, int64_t ldc, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(M, RNN_GEMM_M), (unsigned)cdiv(Nc, RNN_GEMM_N));
  GCRNN_PRE_LAUNCH();
  rnn_gemm_kernel<A><<<grid, RNN_GEMM_THREADS, 0, st>>>(Am, Bm, b1, b2, Cm, M, (int)Nc, (int)K, lda, sbk, sbn, ldc);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <typename A, int FP>
int rnn_forward_t(const A* x, const A* h0, const A* wih, const A* whh, const A* bih, const A* bhh, A* H, const RnnLayout& L,
                  int64_t B, int64_t T, int64_t D, int64_t Fh, int relu, hipStream_t st) {
  int s = rnn_gemm<A>(x, wih, bih, bhh, H, L.rows, Fh, D, D, 1, D, Fh, st);
  if (s != GCRNN_OK) return s;
  GCRNN_PRE_LAUNCH();
  rnn_forward_kernel<A, FP><<<(unsigned)B, 64, 0, st>>>(h0, whh, H, (int)T, (int)Fh, relu);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <typename A, int FP>
int rnn_backward_t(const A* x, const A* h0, const A* wih, const A* whh, const A* H, const A* dH, A* dZ, A* dh0, A* dx, A* parts,
                   const RnnLayout& L, int64_t B, int64_t T, int64_t D, int64_t Fh, int relu, hipStream_t st) {
  GCRNN_PRE_LAUNCH();
  rnn_bptt_kernel<A, FP><<<(unsigned)B, 64, 0, st>>>(whh, H, dH, dZ, dh0, (int)T, (int)Fh, relu);
  GCRNN_CHECK_LAUNCH();
  GCRNN_PRE_LAUNCH();
  rnn_wgrad_kernel<A, FP><<<dim3((unsigned)L.col_tiles, (unsigned)L.slots), RNN_WG_THREADS, 0, st>>>(x, h0, H, dZ, parts, L.rows,
                                                                                                    L.rows_per_slot, (int)T, (int)D,
                                                                                                    (int)Fh);
  GCRNN_CHECK_LAUNCH();
  if (dx) return rnn_gemm<A>(dZ, wih, nullptr, nullptr, dx, L.rows, D, Fh, Fh, D, 1, D, st);
  return GCRNN_OK;
}

template <typename A>
int rnn_forward_d(const void* x, const void* h0, const void* wih, const void* whh, const void* bih, const void* bhh, void* H,
                  const RnnLayout& L, int64_t B, int64_t T, int64_t D, int64_t Fh, int relu, hipStream_t st) {
#define RNN_FWD(FP)                                                                                                              \
  return rnn_forward_t<A, FP>((const A*)x, (const A*)h0, (const A*)wih, (const A*)whh, (const A*)bih, (const A*)bhh, (A*)H, L, B, \
                              T, D, Fh, relu, st)
  switch (L.fh_pad) {
    case 4: RNN_FWD(4);
    case 8: RNN_FWD(8);
    case 16: RNN_FWD(16);
    case 32: RNN_FWD(32);
    default: RNN_FWD(64);
  }
#undef RNN_FWD
}

template <typename A>
int rnn_backward_d(const void* x, const void* h0, const void* wih, const void* whh, const void* H, const void* dH, void* dZ,
                   void* dh0, void* dx, void* parts, const RnnLayout& L, int64_t B, int64_t T, int64_t D, int64_t Fh, int relu,
                   hipStream_t st) {
#define RNN_BWD(FP)                                                                                                             \
  return rnn_backward_t<A, FP>((const A*)x, (const A*)h0, (const A*)wih, (const A*)whh, (const A*)H, (const A*)dH, (A*)dZ,      \
                               (A*)dh0, (A*)dx, (A*)parts, L, B, T, D, Fh, relu, st)
  switch (L.fh_pad) {
    case 4: RNN_BWD(4);
    case 8: RNN_BWD(8);
    case 16: RNN_BWD(16);
    case 32: RNN_BWD(32);
    default: RNN_BWD(64);
  }
#undef RNN_BWD
}

int rnn_check(int dtype, int64_t B, int64_t T, int64_t D, int64_t Fh, int act) {
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return GCRNN_ERR_BAD_DTYPE;
  if (B <= 0 || T <= 0 || D <= 0 || Fh <= 0 || act < 0 || act > 1) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_rnn_supported(dtype, B, T, D, Fh)) return GCRNN_ERR_UNSUPPORTED;
  return GCRNN_OK;
}

}  // namespace

extern "C" int gcrnn_rnn_forward(int dtype, const void* x, const void* h0, const void* w_ih, const void* w_hh, const void* b_ih,
                                 const void* b_hh, void* H, int64_t B, int64_t T, int64_t D, int64_t F_h, int act, void* stream) {
  if (!x || !h0 || !w_ih || !w_hh || !H || (!b_ih) != (!b_hh)) return GCRNN_ERR_NULL_POINTER;
  const int st = rnn_check(dtype, B, T, D, F_h, act);
  if (st != GCRNN_OK) return st;
  const RnnLayout L = rnn_layout(B, T, D, F_h);
  hipStream_t s = as_stream(stream);
  if (dtype == GCRNN_F32) return rnn_forward_d<float>(x, h0, w_ih, w_hh, b_ih, b_hh, H, L, B, T, D, F_h, act, s);
  return rnn_forward_d<double>(x, h0, w_ih, w_hh, b_ih, b_hh, H, L, B, T, D, F_h, act, s);
}

extern "C" int gcrnn_rnn_backward(int dtype, const void* x, const void* h0, const void* w_ih, const void* w_hh, const void* H,
                                  const void* dH, void* dZ, void* dh0, void* dx, void* dw_parts, int64_t slots, int64_t B, int64_t T,
                                  int64_t D, int64_t F_h, int act, void* stream) {
  if (!x || !h0 || !w_ih || !w_hh || !H || !dH || !dZ || !dw_parts) return GCRNN_ERR_NULL_POINTER;
  const int st = rnn_check(dtype, B, T, D, F_h, act);
  if (st != GCRNN_OK) return st;
  if (slots != gcrnn_rnn_wgrad_slots(dtype, B, T, D, F_h)) return GCRNN_ERR_WORKSPACE;
  const RnnLayout L = rnn_layout(B, T, D, F_h);
  hipStream_t s = as_stream(stream);
  if (dtype == GCRNN_F32) return rnn_backward_d<float>(x, h0, w_ih, w_hh, H, dH, dZ, dh0, dx, dw_parts, L, B, T, D, F_h, act, s);
  return rnn_backward_d<double>(x, h0, w_ih, w_hh, H, dH, dZ, dh0, dx, dw_parts, L, B, T, D, F_h, act, s);
}
