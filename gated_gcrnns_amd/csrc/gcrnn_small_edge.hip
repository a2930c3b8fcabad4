// Small-graph regime, EDGE-gated cell (spatial_gating = 'edge', optionally time-gated too), inference: the whole recurrence of one
// sequence runs inside ONE workgroup in ONE launch with the state in LDS, as small_cell_kernel does for the other cell flavours
// (gcrnn_small.hip). Reference: GGCRNNCell.forward, Utils/graphML.py:2411-2416, with graphAttention, graphML.py:521-627.
//
// One branch (input: u = x_t, taps A, attention `input_attention`; state: u = h_{t-1}, taps B, attention `forget_attention`):
//   z_0 = u, z_k = z_{k-1} S                     (K-1 hops; CSR(S^T) held in LDS; one thread per (channel, node))
//   Wx[:, n] = W (sum_k w_k z_k[:, n] + b)       s1[n] = a1 . Wx[:, n]      s2[m] = a2 . Wx[:, m]
//     -- W and the mixer a = [a1 | a2] are folded into the taps ONCE per launch: rows f < F of `wf` hold W w_k, rows F and F + 1
//        hold a1^T W w_k and a2^T W w_k, so Wx, s1 and s2 come out of one tap pass
//   row m of the support of S + I:  e = LeakyReLU_0.2(s1[n] + s2[m]),  mx[m] = max_n e,  den[m] = sum_n exp(e - mx[m])      (row pass)
//   coef[q] = (S + I)[m][n] * (exp(e - mx[m]) / den[m])   for every edge q = (m -> n) of the transposed support list
//   y[:, n] = relu( sum_{q in column n} coef[q] Wx[:, m_q] )   in the fixed order of the transposed list                    (column pass)
// A row with an empty support never appears in the transposed list: it contributes nothing and its den is never divided by.
// No atomics anywhere: the result is bit-reproducible.
//
// The input branch does not depend on the state. XP = true evaluates it for every (b, t) in one launch of B * T workgroups and
// writes Ya[b][t] = gi_t * y_a; XP = false walks t = 0 .. T-1 with h_t = tanh(Ya[b][t] + gf_t * y_b). Two launches per forward,
// whatever T is.
//
// HEAD (recurrence launch only) puts the model's output head behind the state while it sits in LDS (z_0 = h_t):
//   SE_HEAD_LAST  logits[b][c] = head_w[c] . vec(h_T) + head_b[c]        (classification read-out, one wave per class, behind the loop)
//   SE_HEAD_NODE  y_t[o][n] = node_b[o] + sum_f node_w[o][f] h_t[f][n]   (regression head on every state, one thread per (o, n))
// and `store` (GCRNN_SMALL_STATES_*) says which states still go to H. The stored states keep the bits of HEAD = NONE.
#include "gcrnn_common.h"

namespace {

template <typename T> __device__ __forceinline__ T se_tanh(T v);
template <> __device__ __forceinline__ float se_tanh<float>(float v) { return tanhf(v); }
template <> __device__ __forceinline__ double se_tanh<double>(double v) { return tanh(v); }
template <typename T> __device__ __forceinline__ T se_exp(T v);
template <> __device__ __forceinline__ float se_exp<float>(float v) { return expf(v); }
template <> __device__ __forceinline__ double se_exp<double>(double v) { return exp(v); }

constexpr int SE_THREADS = 1024;
constexpr int SE_PASSES = 4;             // (F + 2) * N <= SE_PASSES * SE_THREADS is checked on the host
constexpr int SE_ROW_LANES = 8;          // lanes that share one support row in the row pass
constexpr int SE_HEAD_NONE = 0, SE_HEAD_LAST = 1, SE_HEAD_NODE = 2;

// y[o][n] of the per-node head from the state in z_0: from the bias, f ascending (node_linear_fwd_kernel's order). The O N threads at the END
// of the workgroup: the hop and tap passes load the low thread indices twice when F N > SE_THREADS.
template <typename T>
__device__ __forceinline__ void se_node_head(const T* __restrict__ z, const T* __restrict__ hwl, T* __restrict__ y, int tid, int N, int F,
                                             int O) {
  const int idx = tid - (SE_THREADS - O * N);
  if (idx >= 0) {
    const int o = idx / N, n = idx - o * N;
    const T* wr = hwl + o * F;
    T acc = hwl[O * F + o];
    for (int f = 0; f < F; ++f) acc += wr[f] * z[f * N + n];
    y[idx] = acc;
  }
}

}  // namespace

template <typename T, bool XP, int HEAD = SE_HEAD_NONE>
__global__ __launch_bounds__(1024) void small_edge_cell_kernel(
    const T* __restrict__ U,          // XP: X [B][Tn][C][N]        else: h0 [B][C][N]  (C = F)
    const T* __restrict__ w,          // [F][K][C] filter taps
    const T* __restrict__ bias,       // [F] or null
    const T* __restrict__ attW,       // [F][F]
    const T* __restrict__ attA,       // [2 F]  a1 | a2
    const T* __restrict__ gate,       // [Tn][B] or null            XP: gi, else: gf
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const T* __restrict__ val,       // CSR(S^T)
    const int32_t* __restrict__ s_rowptr, const int2* __restrict__ r_edge,                                // support rows: {n, .}
    const int32_t* __restrict__ t_rowptr, const int2* __restrict__ t_edge, const T* __restrict__ t_val,   // support columns: {m, .}, (S + I)[m][n]
    T* __restrict__ Ya,               // [B][Tn][F][N]              XP: written, else: read
    T* __restrict__ H,                // [B][Tn][F][N] or, last_only, [B][1][F][N]   (not XP); with a head: by `last_only` = GCRNN_SMALL_STATES_*
    const T* __restrict__ head_w,     // HEAD_LAST: [NC][F N]       HEAD_NODE: [NC][F]
    const T* __restrict__ head_b,     // [NC] or null
    T* __restrict__ Y,                // HEAD_LAST: logits [B][NC]  HEAD_NODE: [B][Tn][NC][N]
    int Tn, int N, int C, int F, int K, int nnz, int nnzs, int B, int last_only, int NC) {
  static_assert(!XP || HEAD == SE_HEAD_NONE, "the heads read the state: recurrence launch only");
  extern __shared__ __attribute__((aligned(16))) char smem_small_edge[];
  const int R = F + 2;                                       // rows of the folded taps: Wx | s1 | s2
  T* z = reinterpret_cast<T*>(smem_small_edge);              // [K][C][N]
  T* wf = z + (size_t)K * C * N;                             // [R][K][C]
  T* bf = wf + (size_t)R * K * C;                            // [R]
  T* wx = bf + R;                                            // [R][N]: Wx rows, then s1, then s2
  T* mx = wx + (size_t)R * N;                                // [N]
  T* den = mx + N;                                           // [N]
  T* coef = den + N;                                         // [nnzs]
  T* tvl = coef + nnzs;                                      // [nnzs]
  T* vall = tvl + nnzs;                                      // [nnz]
  T* hwl = vall + nnz;                                       // HEAD_NODE: [NC][F] node_w, then [NC] node_b (0 without one)
  int32_t* rpl = reinterpret_cast<int32_t*>(HEAD == SE_HEAD_NODE ? hwl + NC * (F + 1) : hwl);   // [N + 1]
  int32_t* rrp = rpl + (N + 1);                              // [N + 1]
  int32_t* trp = rrp + (N + 1);                              // [N + 1]
  int32_t* coll = trp + (N + 1);                             // [nnz]
  int32_t* rcol = coll + nnz;                                // [nnzs]
  int32_t* tm = rcol + nnzs;                                 // [nnzs] row m of transposed-list edge q
  int32_t* tn = tm + nnzs;                                   // [nnzs] column n of transposed-list edge q
  const int tid = threadIdx.x;
  const int b = XP ? (int)(blockIdx.x / (unsigned)Tn) : (int)blockIdx.x;
  const int t_first = XP ? (int)(blockIdx.x - (unsigned)b * (unsigned)Tn) : 0;
  const int KC = K * C, CN = C * N, FN = F * N, RN = R * N;
  const T* s1 = wx + (size_t)F * N;
  const T* s2 = s1 + N;

  for (int i = tid; i < nnz; i += SE_THREADS) { vall[i] = val[i]; coll[i] = col[i]; }
  for (int i = tid; i < nnzs; i += SE_THREADS) { tvl[i] = t_val[i]; rcol[i] = r_edge[i].x; tm[i] = t_edge[i].x; }
  for (int i = tid; i <= N; i += SE_THREADS) { rpl[i] = rowptr[i]; rrp[i] = s_rowptr[i]; trp[i] = t_rowptr[i]; }
  // fold the attention's mixing matrix into the taps: wf[f] = W w  (rows f < F)
  for (int i = tid; i < F * KC; i += SE_THREADS) {
    const int f = i / KC, r = i - f * KC;
    T acc = T(0);
    for (int f2 = 0; f2 < F; ++f2) acc += attW[f * F + f2] * w[(size_t)f2 * KC + r];
    wf[i] = acc;
  }
  for (int f = tid; f < F; f += SE_THREADS) {
    T acc = T(0);
    if (bias)
      for (int f2 = 0; f2 < F; ++f2) acc += attW[f * F + f2] * bias[f2];
    bf[f] = acc;
  }
  if (HEAD == SE_HEAD_NODE) {
    for (int i = tid; i < NC * F; i += SE_THREADS) hwl[i] = head_w[i];
    for (int i = tid; i < NC; i += SE_THREADS) hwl[NC * F + i] = head_b ? head_b[i] : T(0);
  }
  if (!XP)
    for (int i = tid; i < FN; i += SE_THREADS) z[i] = U[(size_t)b * FN + i];                    // z_0 = h0
  __syncthreads();
  // ... and the mixer: rows F, F + 1 = a1^T (W w), a2^T (W w)
  for (int i = tid; i < 2 * KC; i += SE_THREADS) {
    const int h = i / KC, r = i - h * KC;
    T acc = T(0);
    for (int f = 0; f < F; ++f) acc += attA[h * F + f] * wf[f * KC + r];
    wf[(F + h) * KC + r] = acc;
  }
  if (tid < 2) {
    T acc = T(0);
    for (int f = 0; f < F; ++f) acc += attA[tid * F + f] * bf[f];
    bf[F + tid] = acc;
  }
  for (int n = tid; n < N; n += SE_THREADS)
    for (int q = trp[n]; q < trp[n + 1]; ++q) tn[q] = n;
  // (the first barrier of the step loop orders these writes before their readers)

  // outputs this thread owns in the tap pass (R N of them) and, as the first F N of those, in the column pass
  int of[SE_PASSES], on[SE_PASSES];
#pragma unroll
  for (int p = 0; p < SE_PASSES; ++p) {
    const int i = tid + p * SE_THREADS;
    of[p] = i / N;
    on[p] = i - of[p] * N;
  }
  const int row_lane = tid & (SE_ROW_LANES - 1);

  const int t_end = XP ? t_first + 1 : Tn;
  for (int t = t_first; t < t_end; ++t) {
    T ya[SE_PASSES];
    if (XP) {
      const T* xt = U + ((size_t)b * Tn + t) * CN;
      for (int i = tid; i < CN; i += SE_THREADS) z[i] = xt[i];                                  // z_0 = x_t
    } else {
      // the input branch of this step, fetched before the step's work so that its latency hides behind it
      const T* yat = Ya + ((size_t)b * Tn + t) * FN;
#pragma unroll
      for (int p = 0; p < SE_PASSES; ++p) {
        const int i = tid + p * SE_THREADS;
        ya[p] = (i < FN) ? yat[i] : T(0);
      }
    }
    __syncthreads();
    // y_{t-1}: h_{t-1} is stable in z_0 from this barrier until the step's column pass writes h_t over it
    if (HEAD == SE_HEAD_NODE && t > 0) se_node_head<T>(z, hwl, Y + ((size_t)b * Tn + (t - 1)) * NC * N, tid, N, F, NC);
    for (int k = 1; k < K; ++k) {                                                               // z_k = z_{k-1} S
      const T* zp = z + (size_t)(k - 1) * CN;
      T* zn = z + (size_t)k * CN;
      for (int i = tid; i < CN; i += SE_THREADS) {
        const int c = i / N, n = i - c * N;
        const T* zr = zp + c * N;
        T acc = T(0);
        for (int j = rpl[n]; j < rpl[n + 1]; ++j) acc += vall[j] * zr[coll[j]];
        zn[i] = acc;
      }
      __syncthreads();
    }
    // ---- taps: Wx, s1, s2 in one pass
#pragma unroll
    for (int p = 0; p < SE_PASSES; ++p) {
      const int i = tid + p * SE_THREADS;
      if (i < RN) {
        const T* wr = wf + of[p] * KC;
        const T* zc = z + on[p];
        T acc = bf[of[p]];
        for (int kc = 0; kc < KC; ++kc) acc += wr[kc] * zc[kc * N];
        wx[i] = acc;
      }
    }
    __syncthreads();
    // ---- row pass: SE_ROW_LANES lanes per support row, butterfly reductions in a fixed order
    for (int m = tid / SE_ROW_LANES; m < N; m += SE_THREADS / SE_ROW_LANES) {
      const int j0 = rrp[m], j1 = rrp[m + 1];
      const T z2 = s2[m];
      T mv = (T)(-INFINITY);
      for (int j = j0 + row_lane; j < j1; j += SE_ROW_LANES) {
        const T zz = s1[rcol[j]] + z2;
        const T e = zz > T(0) ? zz : T(0.2) * zz;
        mv = e > mv ? e : mv;
      }
#pragma unroll
      for (int o = SE_ROW_LANES / 2; o > 0; o >>= 1) {
        const T other = __shfl_xor(mv, o, SE_ROW_LANES);
        mv = other > mv ? other : mv;
      }
      T d = T(0);
      for (int j = j0 + row_lane; j < j1; j += SE_ROW_LANES) {
        const T zz = s1[rcol[j]] + z2;
        const T e = zz > T(0) ? zz : T(0.2) * zz;
        d += se_exp<T>(e - mv);
      }
#pragma unroll
      for (int o = SE_ROW_LANES / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, SE_ROW_LANES);
      if (row_lane == 0) { mx[m] = mv; den[m] = d; }
    }
    __syncthreads();
    // ---- one coefficient per edge of the transposed list
    for (int q = tid; q < nnzs; q += SE_THREADS) {
      const int m = tm[q];
      const T zz = s1[tn[q]] + s2[m];
      const T e = zz > T(0) ? zz : T(0.2) * zz;
      coef[q] = tvl[q] * (se_exp<T>(e - mx[m]) / den[m]);
    }
    __syncthreads();
    // ---- column pass and the step's epilogue
    T g = T(1);
    if (gate) g = gate[(size_t)t * B + b];
    bool store;
    T* out;
    if (HEAD == SE_HEAD_NONE) {
      store = XP || !last_only || t == Tn - 1;
      out = XP ? Ya + ((size_t)b * Tn + t) * FN : H + ((size_t)b * (last_only ? 1 : Tn) + (last_only ? 0 : t)) * FN;
    } else {                                                                                    // last_only: GCRNN_SMALL_STATES_*
      store = last_only == GCRNN_SMALL_STATES_ALL || (last_only == GCRNN_SMALL_STATES_LAST && t == Tn - 1);
      out = last_only == GCRNN_SMALL_STATES_ALL ? H + ((size_t)b * Tn + t) * FN : H + (size_t)b * FN;      // (never dereferenced with _NONE)
    }
#pragma unroll
    for (int p = 0; p < SE_PASSES; ++p) {
      const int i = tid + p * SE_THREADS;
      if (i < FN) {
        const int n = on[p];
        const T* wr = wx + of[p] * N;
        T acc = T(0);
        for (int q = trp[n]; q < trp[n + 1]; ++q) acc += coef[q] * wr[tm[q]];
        const T y = g * (acc <= T(0) ? T(0) : acc);      // (relu as torch has it: a NaN stays a NaN)
        if (XP) {
          out[i] = y;
        } else {
          const T h = se_tanh<T>(ya[p] + y);
          if (store) out[i] = h;
          z[i] = h;                   // z_0 = h_t (C = F): every reader of z_0 in this step is behind two barriers
        }
      }
    }
    // the next step's first barrier orders the new state before the hops that read it
  }
  if (HEAD != SE_HEAD_NONE) {
    __syncthreads();                                                                            // h_T in z_0
    if (HEAD == SE_HEAD_NODE) {
      se_node_head<T>(z, hwl, Y + ((size_t)b * Tn + (Tn - 1)) * NC * N, tid, N, F, NC);
    } else {
      // one wave per class, lanes stride over i = f N + n; the 64 partial sums fold in a fixed xor butterfly
      const int lane = tid & 63;
      for (int c = tid >> 6; c < NC; c += SE_THREADS / 64) {
        const T* wr = head_w + (size_t)c * FN;
        T acc = T(0);
        for (int i = lane; i < FN; i += 64) acc += wr[i] * z[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) Y[(size_t)b * NC + c] = acc + (head_b ? head_b[c] : T(0));
      }
    }
  }
}

static size_t small_edge_lds_bytes(int dtype, int64_t N, int64_t nnz, int64_t nnzs, int64_t G, int64_t F, int64_t Kin, int64_t Kst) {
  const size_t e = dtype == GCRNN_F64 ? 8 : 4;
  const int64_t K = Kin > Kst ? Kin : Kst, C = G > F ? G : F, R = F + 2;
  return e * (size_t)(K * C * N + R * K * C + R + R * N + 2 * N + 2 * nnzs + nnz) + 4 * (size_t)(3 * (N + 1) + nnz + 3 * nnzs) + 16;
}

extern "C" int gcrnn_small_edge_supported(int dtype, int64_t N, int64_t nnz, int64_t nnz_support, int64_t G, int64_t F,
                                          int64_t Kin, int64_t Kst) {
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return 0;
  if (N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0 || nnz < 0 || nnz_support < 0) return 0;
  // N: what one pass of the row phase covers (128), the regime this path was measured in (the drivers' N = 50 .. 80); larger graphs
  // keep the paths they have
  if (N > SE_THREADS / SE_ROW_LANES || G > 1024 || F > 1024 || Kin > 64 || Kst > 64 || nnz > N * N || nnz_support > N * N) return 0;
  if ((F + 2) * N > SE_PASSES * SE_THREADS) return 0;
  return small_edge_lds_bytes(dtype, N, nnz, nnz_support, G, F, Kin, Kst) <= 150 * 1024 ? 1 : 0;
}

// the LDS values of the head: node_w | node_b of the per-node head; the read-out streams head_w from global memory
static size_t small_edge_head_lds_bytes(int dtype, int head_kind, int64_t F, int64_t NC) {
  return head_kind == SE_HEAD_NODE ? (dtype == GCRNN_F64 ? 8 : 4) * (size_t)(NC * (F + 1)) : 0;
}

extern "C" int gcrnn_small_edge_head_supported(int dtype, int64_t N, int64_t nnz, int64_t nnz_support, int64_t G, int64_t F,
                                               int64_t Kin, int64_t Kst, int head_kind, int64_t NC, int backward) {
  if (!gcrnn_small_edge_supported(dtype, N, nnz, nnz_support, G, F, Kin, Kst)) return 0;
  if (backward && !gcrnn_small_edge_backward_supported(dtype, N, nnz, nnz_support, G, F, Kin, Kst)) return 0;
  if (head_kind == SE_HEAD_LAST) {
    if (NC < 1 || NC > GCRNN_SMALL_HEAD_MAX_CLASSES) return 0;
  } else if (head_kind == SE_HEAD_NODE) {
    if (NC < 1 || NC > GCRNN_SMALL_NODE_HEAD_MAX_OUT) return 0;          // O N <= 8 * 128 threads: one per (o, n)
  } else {
    return 0;
  }
  return small_edge_lds_bytes(dtype, N, nnz, nnz_support, G, F, Kin, Kst) + small_edge_head_lds_bytes(dtype, head_kind, F, NC) <= 150 * 1024
             ? 1 : 0;
}

namespace {
struct SmallEdgeFwdArgs {
  const void *X, *h0, *wA, *wB, *bias, *att_in_w, *att_in_a, *att_f_w, *att_f_a, *gi, *gf;
  const int32_t *rowptr, *col;
  const void* val;
  const int32_t *s_rowptr, *r_edge, *t_rowptr, *t_edge;
  const void* t_val;
  void *Ya, *H;
  const void *head_w, *head_b;
  void* Y;
  int64_t B, T, N, G, F, Kin, Kst, nnz, nnzs, NC;
  int store;                            // HEAD_NONE: last_only; with a head: GCRNN_SMALL_STATES_*
};
}  // namespace

template <typename T, int HEAD>
static int small_edge_launch(const SmallEdgeFwdArgs& a, size_t lds, hipStream_t st) {
  auto kx = small_edge_cell_kernel<T, true>;
  auto kh = small_edge_cell_kernel<T, false, HEAD>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(kh), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kx<<<(unsigned)(a.B * a.T), SE_THREADS, lds, st>>>((const T*)a.X, (const T*)a.wA, (const T*)a.bias, (const T*)a.att_in_w,
                                                     (const T*)a.att_in_a, (const T*)a.gi, a.rowptr, a.col, (const T*)a.val, a.s_rowptr,
                                                     (const int2*)a.r_edge, a.t_rowptr, (const int2*)a.t_edge, (const T*)a.t_val, (T*)a.Ya,
                                                     (T*)nullptr, (const T*)nullptr, (const T*)nullptr, (T*)nullptr, (int)a.T, (int)a.N,
                                                     (int)a.G, (int)a.F, (int)a.Kin, (int)a.nnz, (int)a.nnzs, (int)a.B, 0, 0);
  kh<<<(unsigned)a.B, SE_THREADS, lds, st>>>((const T*)a.h0, (const T*)a.wB, (const T*)a.bias, (const T*)a.att_f_w, (const T*)a.att_f_a,
                                             (const T*)a.gf, a.rowptr, a.col, (const T*)a.val, a.s_rowptr, (const int2*)a.r_edge,
                                             a.t_rowptr, (const int2*)a.t_edge, (const T*)a.t_val, (T*)a.Ya, (T*)a.H, (const T*)a.head_w,
                                             (const T*)a.head_b, (T*)a.Y, (int)a.T, (int)a.N, (int)a.F, (int)a.F, (int)a.Kst, (int)a.nnz,
                                             (int)a.nnzs, (int)a.B, a.store, (int)a.NC);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// both entry points: the validation, then the two launches. Without `head` it is gcrnn_small_edge_forward (store = last_only).
static int small_edge_forward(int dtype, const SmallEdgeFwdArgs& a, bool head, int head_kind, void* stream) {
  if (!a.X || !a.h0 || !a.wA || !a.wB || !a.att_in_w || !a.att_in_a || !a.att_f_w || !a.att_f_a || !a.rowptr || !a.s_rowptr ||
      !a.t_rowptr || !a.Ya)
    return GCRNN_ERR_NULL_POINTER;
  if (!a.H && !(head && a.store == GCRNN_SMALL_STATES_NONE)) return GCRNN_ERR_NULL_POINTER;
  if (head && (!a.head_w || !a.Y)) return GCRNN_ERR_NULL_POINTER;
  if ((a.nnz > 0 && (!a.col || !a.val)) || (a.nnzs > 0 && (!a.r_edge || !a.t_edge || !a.t_val))) return GCRNN_ERR_NULL_POINTER;
  if ((a.gi == nullptr) != (a.gf == nullptr)) return GCRNN_ERR_NULL_POINTER;
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return GCRNN_ERR_BAD_DTYPE;
  if (a.B <= 0 || a.T <= 0 || a.N <= 0 || a.G <= 0 || a.F <= 0 || a.Kin <= 0 || a.Kst <= 0 || a.nnz < 0 || a.nnzs < 0)
    return GCRNN_ERR_BAD_SHAPE;
  if (a.B > 2147483647LL || a.T > 2147483647LL || a.B * a.T > 2147483647LL) return GCRNN_ERR_BAD_SHAPE;
  if (head) {
    if (head_kind != SE_HEAD_LAST && head_kind != SE_HEAD_NODE) return GCRNN_ERR_BAD_SHAPE;
    if (a.store != GCRNN_SMALL_STATES_ALL && a.store != GCRNN_SMALL_STATES_LAST && a.store != GCRNN_SMALL_STATES_NONE)
      return GCRNN_ERR_BAD_SHAPE;
    if (a.NC <= 0 || a.NC > (head_kind == SE_HEAD_NODE ? GCRNN_SMALL_NODE_HEAD_MAX_OUT : GCRNN_SMALL_HEAD_MAX_CLASSES))
      return GCRNN_ERR_BAD_SHAPE;
    if (!gcrnn_small_edge_head_supported(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst, head_kind, a.NC, 0))
      return GCRNN_ERR_UNSUPPORTED;
  } else if (!gcrnn_small_edge_supported(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst)) {
    return GCRNN_ERR_UNSUPPORTED;
  }
  const size_t lds = small_edge_lds_bytes(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst) +
                     small_edge_head_lds_bytes(dtype, head_kind, a.F, a.NC);
  hipStream_t st = as_stream(stream);
  if (dtype == GCRNN_F32) {
    if (head_kind == SE_HEAD_LAST) return small_edge_launch<float, SE_HEAD_LAST>(a, lds, st);
    if (head_kind == SE_HEAD_NODE) return small_edge_launch<float, SE_HEAD_NODE>(a, lds, st);
    return small_edge_launch<float, SE_HEAD_NONE>(a, lds, st);
  }
  if (head_kind == SE_HEAD_LAST) return small_edge_launch<double, SE_HEAD_LAST>(a, lds, st);
  if (head_kind == SE_HEAD_NODE) return small_edge_launch<double, SE_HEAD_NODE>(a, lds, st);
  return small_edge_launch<double, SE_HEAD_NONE>(a, lds, st);
}

extern "C" int gcrnn_small_edge_forward(int dtype, const void* X, const void* h0, const void* wA, const void* wB, const void* bias,
                                        const void* att_in_w, const void* att_in_a, const void* att_f_w, const void* att_f_a,
                                        const void* gi, const void* gf, const int32_t* rowptr, const int32_t* col, const void* val,
                                        const int32_t* s_rowptr, const int32_t* r_edge, const int32_t* t_rowptr,
                                        const int32_t* t_edge, const void* t_val, void* Ya, void* H, int64_t B, int64_t T, int64_t N,
                                        int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t nnz, int64_t nnz_support,
                                        int last_only, void* stream) {
  const SmallEdgeFwdArgs a = {X, h0, wA, wB, bias, att_in_w, att_in_a, att_f_w, att_f_a, gi, gf, rowptr, col, val, s_rowptr, r_edge,
                              t_rowptr, t_edge, t_val, Ya, H, nullptr, nullptr, nullptr, B, T, N, G, F, Kin, Kst, nnz, nnz_support, 0,
                              last_only ? 1 : 0};
  return small_edge_forward(dtype, a, false, SE_HEAD_NONE, stream);
}

extern "C" int gcrnn_small_edge_forward_head(int dtype, const void* X, const void* h0, const void* wA, const void* wB, const void* bias,
                                             const void* att_in_w, const void* att_in_a, const void* att_f_w, const void* att_f_a,
                                             const void* gi, const void* gf, const int32_t* rowptr, const int32_t* col, const void* val,
                                             const int32_t* s_rowptr, const int32_t* r_edge, const int32_t* t_rowptr,
                                             const int32_t* t_edge, const void* t_val, void* Ya, void* H, const void* head_w,
                                             const void* head_b, void* Y, int64_t B, int64_t T, int64_t N, int64_t G, int64_t F,
                                             int64_t Kin, int64_t Kst, int64_t nnz, int64_t nnz_support, int64_t NC, int head_kind,
                                             int store_states, void* stream) {
  const SmallEdgeFwdArgs a = {X, h0, wA, wB, bias, att_in_w, att_in_a, att_f_w, att_f_a, gi, gf, rowptr, col, val, s_rowptr, r_edge,
                              t_rowptr, t_edge, t_val, Ya, H, head_w, head_b, Y, B, T, N, G, F, Kin, Kst, nnz, nnz_support, NC,
                              store_states};
  return small_edge_forward(dtype, a, true, head_kind, stream);
}
