// Small-graph regime on the fp64 / fp32 matrix cores (BASELINE configs[0], [3]; the drivers' N = 50..80).
//
// With N <= ~128 nodes the GSO fits in LDS as a DENSE N x N matrix, and every piece of a time step is a small GEMM:
//   hop      Z_k   [C x N]  = Z_{k-1} [C x N] * S [N x N]                     (reference x @ S, graphML.py:123)
//   taps     pre   [F x N]  = W [F x K C] * Zflat [K C x N]                   (graphML.py:134-135)
//   dW       [F x C] per tap += dpre [F x N] * Z_k^T [N x C]
//   adjoint  carry [F x N]  = sum_k (B_k^T dpre) (S^T)^k   (Horner: acc <- acc S^T + B_k^T dpre)
// so the whole T-step recurrence (and its BPTT) of one sequence runs in ONE workgroup, ONE launch, on
// v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 with operands read straight from LDS. The gather-based kernels of
// gcrnn_small.hip spend 12.5 us (forward) / 21 us (backward) per time step on LDS instruction issue; here a step is a few
// hundred MFMAs. Everything stays channel-major [c][n] = the user layout, so x_t / H rows move as contiguous segments.
//
// LDS row stride: every matrix uses a stride whose byte size is an ODD multiple of 16 (mod 256). Then the pattern
// "16 lanes over 16 rows, 4 lane groups over 4 consecutive elements" (A operands, transposed B operands) is conflict-free
// and the pattern "16 lanes over 16 consecutive elements, 4 lane groups over 4 rows" costs 2x the minimum.
//
// Register layouts (probed on gfx950, tools/probes/mfma_layout_probe.hip): A[i][k] in lane i + 16 k, B[k][j] in lane
// j + 16 k; D[i][j]: column j = lane % 16, row i = 4 (lane / 16) + r for fp32 but (lane / 16) + 4 r for fp64.
#include "gcrnn_common.h"
#include "gcrnn_small_mfma.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
// MODE = FWD_PLAIN is the plain recurrence that stores every state (head_w / head_b / logits / NC / store are ignored and cost it nothing);
// MODE = FWD_LAST adds the choice of stored states and the read-out on the last state; MODE = FWD_NODE has the choice of stored states and
// the per-node head on EVERY state: Y[b][t][o][n] = sum_f node_w[o][f] h_t[f][n] + node_b[o] (f ascending), with node_w / node_b / Y / O in
// the places of head_w / head_b / logits / NC. The per-step arithmetic is the same code; the mode is a template parameter because a runtime
// head branch costs the MAXT = 4 instantiations scratch. MODE = FWD_GNN has the choice of stored states and a one-layer graph-filter head
// on EVERY state: Y[b][t][0][n] = act(head_b + sum_{k < NC} sum_f head_w[k][f] (h_t S^k)[f][n]) (k ascending, f ascending), NC = K_o its
// number of taps. (h_t S^k) are the state rows of hop level k of step t + 1, so the head shifts nothing of its own while K_o <= K; the
// levels K .. K_o - 1 are shifted for the state rows alone into ZX, outside the rows the tap MFMAs read. MODE = FWD_CLS_GNN has the choice
// of stored states and, on the LAST state only, that graph-filter head followed by a read-out Linear(N -> NL): v[n] = act(head_b + sum_k
// sum_f head_w[k][f] (h_T S^k)[f][n]), logits[b][c] = lin_b[c] + sum_n lin_w[c][n] v[n] (the classification model's Selection-GNN head).
// Its time loop is the plain one; the head is FWD_GNN's epilogue into an LDS vector and FWD_LAST's wave-per-class read-out over it.
enum { FWD_PLAIN = 0, FWD_LAST = 1, FWD_NODE = 2, FWD_GNN = 3, FWD_CLS_GNN = 4 };

// the graph-filter layer's activations in its codes (ops._GFL_ACTS): 0 identity, 1 ReLU, 2 tanh, 3 sigmoid
template <typename T> __device__ __forceinline__ T dense_gnn_act(T v, int act) {
  if (act == 1) return v <= T(0) ? T(0) : v;      // (as torch.relu: a NaN stays a NaN)
  if (act == 2) return tanh(v);
  if (act == 3) return T(1) / (T(1) + exp(-v));
  return v;
}

template <typename T, int MAXT, int MODE>
__global__ __launch_bounds__(1024) void small_dense_fwd_kernel(
    const T* __restrict__ X,       // [B][Tn][G][N]
    const T* __restrict__ h0,      // [B][F][N]
    const T* __restrict__ wA,      // [F][Kin][G]
    const T* __restrict__ wB,      // [F][Kst][F]
    const T* __restrict__ bias,    // [F] or null
    const T* __restrict__ gi, const T* __restrict__ gf,       // gates of the input / state filter per (b, t, n) through strides, or null
    const T* __restrict__ Sd,      // [N][N] dense S (row m, column n)
    T* __restrict__ H,             // [B][Tn][F][N] (store == 0), [B][1][F][N] (store == 1) or unused (store == 2)
    int Tn, int N, int G, int F, int Kin, int Kst, int B,
    int64_t gsb, int64_t gst, int64_t gsn,       // gate element (b, t, n) sits at b gsb + t gst + n gsn
    const T* __restrict__ head_w,  // [NC][F N] read-out on the last state (nn.Linear weight, row-major over (f, n)) or null | FWD_NODE, FWD_GNN: [NC][F]
    const T* __restrict__ head_b,  // [NC] or null | FWD_GNN: [1] or null
    T* __restrict__ logits,        // [B][NC] (with head_w) | FWD_NODE: Y [B][Tn][NC][N] | FWD_GNN: Y [B][Tn][1][N] | FWD_CLS_GNN: [B][NL]
    int NC, int store,             // store: GCRNN_SMALL_STATES_ALL / _LAST / _NONE
    int act,                       // FWD_GNN, FWD_CLS_GNN: the head's activation (dense_gnn_act)
    const T* __restrict__ lin_w,   // FWD_CLS_GNN: [NL][N] the read-out behind the graph-filter head (the other modes ignore these four)
    const T* __restrict__ lin_b,   //              [NL] or null
    T* __restrict__ V,             //              [B][N] the head's output on the last state, or null (the training forward keeps it)
    int NL) {
  constexpr bool EXT = MODE != FWD_PLAIN;
  typedef typename Mf<T>::acc acc_t;
  extern __shared__ __attribute__((aligned(16))) char smem_dense[];
  const int K = Kin > Kst ? Kin : Kst;
  const int C = G + F, KC = K * C;
  const int Ns = lds_stride<T>(N), KCs = lds_stride<T>(KC);
  const int N4 = (N + 3) & ~3, KC4 = (KC + 3) & ~3;
  T* S = reinterpret_cast<T*>(smem_dense);         // [N4][Ns]
  T* Z = S + (size_t)N4 * Ns;                      // [KC4][Ns]  (level k = rows k C .. k C + C - 1)
  T* W = Z + (size_t)KC4 * Ns;                     // [F16][KCs] combined taps, F16 = F rounded up to 16
  const int F16 = (F + 15) & ~15;
  T* zrow = W + (size_t)F16 * KCs;                 // [Ns] zeros: what masked lanes read
  T* gvec = zrow + Ns;                             // [2][Ns] gates of this step: input-filter | state-filter, per node
  T* hw = gvec + 2 * Ns;                           // FWD_NODE: [NC][F + 1] the head's weights, its bias in column F (dense_node_head_lds)
                                                   // FWD_GNN, FWD_CLS_GNN: [NC][F] the head's taps, then its bias (dense_gnn_head_lds)
  const int F4 = (F + 3) & ~3;
  T* ZX = hw + ((NC * F + 1 + 3) & ~3);            // FWD_GNN, FWD_CLS_GNN: [NC - K][F4][Ns] state rows of the hop levels K .. NC - 1
  T* vv = ZX + (size_t)(NC > K ? NC - K : 0) * F4 * Ns;      // FWD_CLS_GNN: [Ns] the head's output on the last state (dense_cls_gnn_head_lds)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int b = blockIdx.x;
  // FWD_NODE: y_t from h_t in rows G .. G+F-1 of Z, one thread per (o, n) -- consecutive n on consecutive LDS words, hw[o] a broadcast.
  // The threads are taken from the END of the block: the hop and tap tiles are dealt from wave 0 up, so the last waves have the least to do.
  // It runs between the barrier on top of step t + 1 and the barrier behind that step's taps, where nothing writes those rows.
  auto node_head = [&](int t) {
    T* yt = logits + ((size_t)b * Tn + t) * NC * N;
    for (int i = 1023 - tid; i < NC * N; i += 1024) {
      const int o = i / N, n = i - o * N;
      const T* wr = hw + o * (F + 1);
      T s = wr[F];                      // the accumulator starts from the bias and takes f in ascending order, as node_linear_fwd_kernel does
      const T* zr = Z + G * Ns + n;
      int f = 0;
      for (; f + 4 <= F; f += 4) {      // eight LDS reads in flight in front of the four dependent multiply-adds (tile_mac's batching)
        const T w0 = wr[f], w1 = wr[f + 1], w2 = wr[f + 2], w3 = wr[f + 3];
        const T z0 = zr[f * Ns], z1 = zr[(f + 1) * Ns], z2 = zr[(f + 2) * Ns], z3 = zr[(f + 3) * Ns];
        s += w0 * z0;
        s += w1 * z1;
        s += w2 * z2;
        s += w3 * z3;
      }
      for (; f < F; ++f) s += wr[f] * zr[f * Ns];
      yt[i] = s;
    }
  };

  // FWD_GNN: the state rows of hop level k (rows k C + G .. of Z, or ZX beyond the cell's own levels), and the hop of those rows alone
  // into level k: the tiles of the state write-back, A = level k - 1 (rows >= F read zeros), B = S.
  auto gnn_level = [&](int k) -> T* { return k < K ? Z + (size_t)(k * C + G) * Ns : ZX + (size_t)(k - K) * F4 * Ns; };
  auto gnn_state_hop = [&](int k) {
    const T* zp = gnn_level(k - 1);
    T* zn = gnn_level(k);
    for (int tile = wave; tile < (F16 >> 4) * ((N + 15) >> 4); tile += 16) {
      const int tn = (N + 15) >> 4;
      const int i0 = (tile / tn) << 4, j0 = (tile % tn) << 4;
      acc_t acc = {0, 0, 0, 0};
      const T* ap = (i0 + li < F) ? zp + (i0 + li) * Ns + lk : zrow + lk;
      acc = tile_mac<T>(acc, ap, 4, S + lk * Ns + j0 + li, 4 * Ns, N4 >> 2);
      const int n = j0 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = i0 + Mf<T>::row(lane, r);
        if (f < F && n < N) zn[f * Ns + n] = acc[r];
      }
    }
  };
  // FWD_GNN: y_t from the state rows of all NC levels (gnn_node: one node's value; FWD_CLS_GNN uses it for the last state alone), one thread
  // per node taken from the END of the block as node_head's are. It reads the state rows only -- never the x rows of the same levels, which
  // hold x_{t+1} by then -- and runs after the last hop barrier of step t + 1 and before the barrier behind that step's taps, where nothing
  // writes those rows. From the bias, k ascending, f ascending.
  auto gnn_node = [&](int n) -> T {
    T s = hw[NC * F];
    for (int k = 0; k < NC; ++k) {
      const T* wr = hw + k * F;
      const T* zr = gnn_level(k) + n;
      int f = 0;
      for (; f + 4 <= F; f += 4) {
        const T w0 = wr[f], w1 = wr[f + 1], w2 = wr[f + 2], w3 = wr[f + 3];
        const T z0 = zr[f * Ns], z1 = zr[(f + 1) * Ns], z2 = zr[(f + 2) * Ns], z3 = zr[(f + 3) * Ns];
        s += w0 * z0;
        s += w1 * z1;
        s += w2 * z2;
        s += w3 * z3;
      }
      for (; f < F; ++f) s += wr[f] * zr[f * Ns];
    }
    return dense_gnn_act<T>(s, act);
  };
  auto gnn_head = [&](int t) {
    T* yt = logits + ((size_t)b * Tn + t) * N;
    for (int n = 1023 - tid; n < N; n += 1024) yt[n] = gnn_node(n);
  };

  for (int i = tid; i < N4 * Ns; i += 1024) {
    const int m = i / Ns, n = i - m * Ns;
    S[i] = (m < N && n < N) ? Sd[(size_t)m * N + n] : T(0);
  }
  for (int i = tid; i < KC4 * Ns; i += 1024) Z[i] = T(0);
  for (int i = tid; i < 3 * Ns; i += 1024) zrow[i] = T(0);
  if (MODE == FWD_GNN || MODE == FWD_CLS_GNN) {
    for (int i = tid; i <= NC * F; i += 1024) hw[i] = i < NC * F ? head_w[i] : (head_b ? head_b[0] : T(0));
    for (int i = tid; i < (NC > K ? NC - K : 0) * F4 * Ns; i += 1024) ZX[i] = T(0);
  }
  if (MODE == FWD_NODE)
    for (int i = tid; i < NC * (F + 1); i += 1024) {
      const int o = i / (F + 1), f = i - o * (F + 1);
      hw[i] = f < F ? head_w[(size_t)o * F + f] : (head_b ? head_b[o] : T(0));
    }
  for (int i = tid; i < F16 * KCs; i += 1024) {
    const int f = i / KCs, kc = i - f * KCs;
    T v = T(0);
    if (f < F && kc < KC) {
      const int k = kc / C, c = kc - k * C;
      if (c < G) { if (k < Kin) v = wA[((size_t)f * Kin + k) * G + c]; }
      else       { if (k < Kst) v = wB[((size_t)f * Kst + k) * F + (c - G)]; }
    }
    W[i] = v;
  }
  __syncthreads();
  for (int i = tid; i < F * N; i += 1024) {
    const int f = i / N, n = i - f * N;
    Z[(G + f) * Ns + n] = h0[(size_t)b * F * N + i];
  }

  const int tilesN = (N + 15) >> 4, tilesC = (C + 15) >> 4, tilesF = F16 >> 4;
  const T* xb = X + (size_t)b * Tn * G * N;
  const int GN = G * N;
  // x_t is fetched one step ahead (the first 1024 values in a register) so that its global-memory latency overlaps
  // the previous step instead of sitting in front of a barrier
  const int xg = tid / N, xn = tid - xg * N;
  T xpre = (tid < GN) ? xb[tid] : T(0);
  for (int t = 0; t < Tn; ++t) {
    const T* xt = xb + (size_t)t * GN;
    if (tid < GN) Z[xg * Ns + xn] = xpre;
    for (int i = tid + 1024; i < GN; i += 1024) {
      const int g = i / N, n = i - g * N;
      Z[g * Ns + n] = xt[i];
    }
    if (t + 1 < Tn && tid < GN) xpre = xt[GN + tid];
    if (gi && tid < 2 * N) {
      const int w = tid >= N, n = tid - w * N;
      gvec[w * Ns + n] = (w ? gf : gi)[b * gsb + t * gst + n * gsn];
    }
    __syncthreads();
    if (MODE == FWD_NODE && t > 0) node_head(t - 1);
    // ---- hops: Z_k = Z_{k-1} S
    for (int k = 1; k < K; ++k) {
      const T* zp = Z + (size_t)(k - 1) * C * Ns;
      T* zn = Z + (size_t)k * C * Ns;
      for (int tile = wave; tile < tilesC * tilesN; tile += 16) {
        const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
        acc_t acc = {0, 0, 0, 0};
        const T* ap = (i0 + li < C) ? zp + (i0 + li) * Ns + lk : zrow + lk;
        acc = tile_mac<T>(acc, ap, 4, S + lk * Ns + j0 + li, 4 * Ns, N4 >> 2);
        const int n = j0 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = i0 + Mf<T>::row(lane, r);
          if (c < C && n < N) zn[c * Ns + n] = acc[r];
        }
      }
      __syncthreads();
    }
    if (MODE == FWD_GNN && t > 0) {
      // the levels of h_{t-1} beyond the cell's own, state rows only (NC <= K: none, and no barrier is added to the step)
      for (int k = K; k < NC; ++k) {
        gnn_state_hop(k);
        __syncthreads();
      }
      gnn_head(t - 1);
    }
    // ---- taps: pre = W Zflat (time gates scale the x- and h-columns of W)
    acc_t outv[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
      const int tile = wave + q * 16;
      if (tile >= tilesF * tilesN) break;
      const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
      acc_t acc = {0, 0, 0, 0};
      const T* wr = W + (i0 + li) * KCs + lk;
      acc = tile_mac<T>(acc, wr, 4, Z + lk * Ns + j0 + li, 4 * Ns, KC4 >> 2);          // A(S)x + B(S)h
      T gxn = T(1), ghn = T(1);
      acc_t ax = {0, 0, 0, 0};
      if (gi) {
        // gates multiply the two filters separately: the input filter's share is the (few) x-columns k C + g again
        const int n = j0 + li;
        gxn = gvec[n < N ? n : 0]; ghn = gvec[Ns + (n < N ? n : 0)];
        for (int k = 0; k < Kin; ++k)
          for (int g0 = 0; g0 < G; g0 += 4) {
            const int g = g0 + lk, gc = g < G ? g : G - 1;
            const T a = (W + (i0 + li) * KCs)[k * C + gc] * (g < G ? T(1) : T(0));
            ax = Mf<T>::mma(a, Z[(k * C + gc) * Ns + j0 + li], ax);
          }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = i0 + Mf<T>::row(lane, r);
        const T bb = (bias && f < F) ? bias[f] : T(0);
        const T pre = gi ? gxn * (ax[r] + bb) + ghn * ((acc[r] - ax[r]) + bb) : acc[r] + T(2) * bb;
        acc[r] = Mf<T>::tanh_(pre);
      }
      outv[q] = acc;
    }
    __syncthreads();                    // every wave is done reading Z_0 (the old state) before it is replaced
    const bool all = !EXT || store == GCRNN_SMALL_STATES_ALL;
    const bool keep = all || (store == GCRNN_SMALL_STATES_LAST && t == Tn - 1);
    T* Hout = H + (all ? (size_t)b * Tn + t : (size_t)b) * F * N;
#pragma unroll
    for (int q = 0; q < MAXT; ++q) {
      const int tile = wave + q * 16;
      if (tile >= tilesF * tilesN) break;
      const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
      const int n = j0 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = i0 + Mf<T>::row(lane, r);
        if (f < F && n < N) {
          const T v = outv[q][r];
          Z[(G + f) * Ns + n] = v;
          if (keep) Hout[(size_t)f * N + n] = v;
        }
      }
    }
    // the x_t copy of the next step touches rows 0..G-1 only; its barrier orders the new state too
  }
  if (MODE == FWD_NODE) {
    __syncthreads();                    // the last state is in Z
    node_head(Tn - 1);
  }
  if (MODE == FWD_GNN) {
    // the last state has no next step whose hops would shift it: its NC - 1 levels are made here, state rows only
    __syncthreads();                    // the last state is in Z
    for (int k = 1; k < NC; ++k) {
      gnn_state_hop(k);
      __syncthreads();
    }
    gnn_head(Tn - 1);
  }
  if (MODE == FWD_CLS_GNN) {
    // ---- graph-filter head and read-out on the last state: FWD_GNN's epilogue into vv, then FWD_LAST's read-out over it
    __syncthreads();                    // the last state is in Z
    for (int k = 1; k < NC; ++k) {
      gnn_state_hop(k);
      __syncthreads();
    }
    for (int n = 1023 - tid; n < N; n += 1024) {
      const T v = gnn_node(n);
      vv[n] = v;
      if (V) V[(size_t)b * N + n] = v;
    }
    __syncthreads();
    // logits[b][c] = lin_w[c] . v + lin_b[c]: one wave per class, lanes stride over n, fixed-order butterfly, lane 0 stores
    for (int c = wave; c < NL; c += 16) {
      const T* wr = lin_w + (size_t)c * N;
      T s = T(0);
      for (int n = lane; n < N; n += 64) s += wr[n] * vv[n];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) logits[(size_t)b * NL + c] = s + (lin_b ? lin_b[c] : T(0));
    }
  }
  if (MODE == FWD_LAST && head_w) {
    // ---- read-out on the last state (rows G .. G+F-1 of Z): logits[b][c] = head_w[c] . vec_{F,N}(h_T) + head_b[c].
    // One wave per class, lanes stride over f N + n (coalesced head_w rows), fixed-order butterfly, lane 0 stores.
    __syncthreads();
    const int FN = F * N;
    for (int c = wave; c < NC; c += 16) {
      const T* wr = head_w + (size_t)c * FN;
      T s = T(0);
      for (int i = lane; i < FN; i += 64) {
        const int f = i / N, n = i - f * N;
        s += wr[i] * Z[(G + f) * Ns + n];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) logits[(size_t)b * NC + c] = s + (head_b ? head_b[c] : T(0));
    }
  }
}

template <typename T>
size_t dense_fwd_lds(int64_t N, int64_t G, int64_t F, int64_t K) {
  const int C = (int)(G + F), KC = (int)K * C;
  const int Ns = lds_stride<T>((int)N), KCs = lds_stride<T>(KC);
  const int N4 = ((int)N + 3) & ~3, KC4 = (KC + 3) & ~3, F16 = ((int)F + 15) & ~15;
  return sizeof(T) * ((size_t)N4 * Ns + (size_t)KC4 * Ns + (size_t)F16 * KCs + 3 * (size_t)Ns) + 16;
}

// ------------------------------------------------------------------------------------------------------------------
// backward (BPTT); same contract as small_cell_bwd_kernel in gcrnn_small.hip
// DX = true also produces dX: the adjoint is one Horner chain over all C = G + F channels,
//   acc [C x N] <- acc S^T + g . (W_k^T dpre),   W_k = [A_k | B_k] [F x C],   g[c][n] = gi[n] (c < G) or gf[n] (c >= G),
// whose rows 0..G-1 are dX_t and whose other rows are carry_{t-1}. The gates depend on the OUTPUT element (row kind, node), so
// they scale the tap product after the MFMA chain; per-node gates (node-gated cells) cost nothing extra. The state taps' image
// WBt [Kst][F4][Fs] is replaced by the combined WT [K][F4][Cs1], the only difference in the LDS need.
// ------------------------------------------------------------------------------------------------------------------
template <typename T, bool GATED, int MAXW, bool DX>
__global__ __launch_bounds__(1024) void small_dense_bwd_kernel(
    const T* __restrict__ X, const T* __restrict__ h0, const T* __restrict__ H, const T* __restrict__ dH,
    const T* __restrict__ wA, const T* __restrict__ wB, const T* __restrict__ bias,
    const T* __restrict__ gi, const T* __restrict__ gf,       // gates per (b, t, n) through strides (GATED)
    const T* __restrict__ Sd,
    T* __restrict__ pA,             // [B][F][Kin][G]
    T* __restrict__ pB,             // [B][F][Kst][F]
    T* __restrict__ pb,             // [B][F]
    T* __restrict__ dgi, T* __restrict__ dgf,                 // [B][Tn][N] gradients of the gates (GATED)
    T* __restrict__ dh0,
    T* __restrict__ dX,             // [B][Tn][G][N] (DX)
    int Tn, int N, int G, int F, int Kin, int Kst, int B,
    int64_t gsb, int64_t gst, int64_t gsn,       // gate element (b, t, n) sits at b gsb + t gst + n gsn (dgi / dgf are dense)
    const T* __restrict__ dlogits,  // dH == null, dY == null: the upstream gradient is that of a read-out on the last state, [B][NC]
    const T* __restrict__ head_w,   //             [NC][F N]   |   with dY: node_w [NC][F]
    int NC,
    const T* __restrict__ dY,       // dH == null: the upstream gradient is that of a per-node head on every state, [B][Tn][NC][N]
    T* __restrict__ dU,             // dH == null, dY == null, dU given: the upstream gradient is that of a graph-filter head + read-out on the
                                    // last state: dlogits [B][NC], lin_w [NC][N], head_w the head's taps [Ko][F]; dU [B][Ko][N] is written
    const T* __restrict__ lin_w, const T* __restrict__ V,     // V [B][N]: the head's output on the last state (the forward's)
    int Ko, int act) {
  typedef typename Mf<T>::acc acc_t;
  extern __shared__ __attribute__((aligned(16))) char smem_dense[];
  const int K = Kin > Kst ? Kin : Kst;
  const int C = G + F;
  const int Ns = lds_stride<T>(N), Fs = lds_stride<T>(F + 1), Cs = lds_stride<T>(C);      // Fs > F: column F of WBt is zero
  const int N4 = (N + 3) & ~3, F4 = (F + 3) & ~3, C4 = (C + 3) & ~3, C16 = (C + 15) & ~15, F16 = (F + 15) & ~15;
  T* S = reinterpret_cast<T*>(smem_dense);         // [max(N4, 16 tilesN)][Ns]   dense S; rows also serve as B operand S[n][m]
  const int tilesN = (N + 15) >> 4, tilesC = C16 >> 4, tilesF = F16 >> 4;
  const int SR = tilesN * 16;                      // rows allocated for S (rows >= N are zero)
  T* Z0 = S + (size_t)SR * Ns;                     // [C4][Ns]  ping
  T* Z1 = Z0 + (size_t)C4 * Ns;                    // [C4][Ns]  pong   (both also hold the adjoint accumulators [F][Ns])
  T* dpre = Z1 + (size_t)C4 * Ns;                  // [F4][Ns]  (rows >= F stay zero: k-padding of the B operands)
  T* carry = dpre + (size_t)F4 * Ns;               // [F4][Ns]
  T* WBt = carry + (size_t)F4 * Ns;                // [Kst][F4 (f)][Fs (f2)]   w_B[f][k][f2]
  const int Cs1 = lds_stride<T>(C + 1);            // DX: WBt holds [K][F4 (f)][Cs1 (c)] = [w_A | w_B][f][k][c], column C zero
  T* WAl = WBt + (DX ? (size_t)K * F4 * Cs1 : (size_t)Kst * F4 * Fs);      // GATED: [F][K][Cs] combined taps
  T* red = WAl + (GATED ? (size_t)F * K * Cs : 0);     // [64]
  T* zrow = red + 64;                                  // [max(Ns, K Cs)] zeros: what masked lanes read
  const int ZR = Ns > K * Cs ? Ns : K * Cs;
  T* gvec = zrow + ZR;                                 // GATED: [2][Ns] gates of this step (input | state filter) per node
  T* gpart = gvec + 2 * Ns;                            // GATED: [2][tilesF][Ns] partial column sums of the gate gradients
  (void)C16; (void)F16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int b = blockIdx.x;

  for (int i = tid; i < SR * Ns; i += 1024) {
    const int m = i / Ns, n = i - m * Ns;
    S[i] = (m < N && n < N) ? Sd[(size_t)m * N + n] : T(0);
  }
  for (int i = tid; i < 2 * C4 * Ns + 2 * F4 * Ns; i += 1024) Z0[i] = T(0);        // Z0, Z1, dpre, carry are contiguous
  for (int i = tid; i < ZR + (GATED ? 2 * Ns + 2 * tilesF * Ns : 0); i += 1024) zrow[i] = T(0);
  if (DX) {
    for (int i = tid; i < K * F4 * Cs1; i += 1024) {
      const int k = i / (F4 * Cs1), rem = i - k * (F4 * Cs1);
      const int f = rem / Cs1, c = rem - f * Cs1;
      T v = T(0);
      if (f < F && c < C) {
        if (c < G) { if (k < Kin) v = wA[((size_t)f * Kin + k) * G + c]; }
        else       { if (k < Kst) v = wB[((size_t)f * Kst + k) * F + (c - G)]; }
      }
      WBt[i] = v;
    }
  } else
  for (int i = tid; i < Kst * F4 * Fs; i += 1024) {
    const int k = i / (F4 * Fs), rem = i - k * (F4 * Fs);
    const int f = rem / Fs, f2 = rem - f * Fs;
    WBt[i] = (f < F && f2 < F) ? wB[((size_t)f * Kst + k) * F + f2] : T(0);
  }
  if (GATED)
    for (int i = tid; i < F * K * Cs; i += 1024) {
      const int f = i / (K * Cs), rem = i - f * (K * Cs);
      const int k = rem / Cs, c = rem - k * Cs;
      T v = T(0);
      if (c < C) {
        if (c < G) { if (k < Kin) v = wA[((size_t)f * Kin + k) * G + c]; }
        else       { if (k < Kst) v = wB[((size_t)f * Kst + k) * F + (c - G)]; }
      }
      WAl[i] = v;
    }
  __syncthreads();

  // weight-gradient accumulator tiles, persistent over t: tile id = (k, fi, cj) -> dW[f][k][c]; wave w owns w, w + 16, ...
  const int wtiles = K * tilesF * tilesC;
  acc_t wacc[MAXW];
#pragma unroll
  for (int q = 0; q < MAXW; ++q) wacc[q] = acc_t{0, 0, 0, 0};
  T bacc = T(0);
  const int FN = F * N, GN = G * N;
  if (!dH && !dY && dU) {
    // graph-filter head + read-out upstream (the classification model's Selection-GNN head): dH_t exists at t = Tn-1 only,
    //   dv[n] = sum_c dlogits[b][c] lin_w[c][n] (c ascending),  dU_0 = dv . act'(V),  dU_k[m] = sum_n dU_{k-1}[n] S[m][n] (n ascending),
    //   dH_T[f][n] = sum_k head_w[k][f] dU_k[n] (k ascending) -> the carry tile, as for the read-out below. Once per sequence: one thread per
    // node. The two levels in flight borrow columns 0 .. N-1 of rows 0 and 1 of Z0 (C >= 2), which the first step's copy of x_t | h_{t-1}
    // overwrites before anything reads them; the padding columns are not touched. Every element of dU[b] is written.
    T* u0 = Z0;
    T* u1 = Z0 + Ns;
    T* dub = dU + (size_t)b * Ko * N;
    for (int n = tid; n < N; n += 1024) {
      T s = T(0);
      for (int c = 0; c < NC; ++c) s += dlogits[(size_t)b * NC + c] * lin_w[(size_t)c * N + n];
      const T d = s * gnn_act_grad<T>(V[(size_t)b * N + n], act);
      u0[n] = d;
      dub[n] = d;
    }
    __syncthreads();
    for (int k = 0; k < Ko; ++k) {
      for (int i = tid; i < FN; i += 1024) {
        const int f = i / N, n = i - f * N;
        const T p = head_w[(size_t)k * F + f] * u0[n];
        carry[f * Ns + n] = k ? carry[f * Ns + n] + p : p;
      }
      if (k + 1 < Ko)
        for (int m = tid; m < N; m += 1024) {
          const T* sr = S + (size_t)m * Ns;
          T s = T(0);
          for (int n = 0; n < N; ++n) s += u0[n] * sr[n];
          u1[m] = s;
          dub[(size_t)(k + 1) * N + m] = s;
        }
      __syncthreads();
      T* tmp = u0; u0 = u1; u1 = tmp;
    }
  } else if (!dH && !dY) {
    // read-out upstream: dH_t exists at t = Tn-1 only, dH_T[f][n] = sum_c dlogits[b][c] head_w[c][f N + n] (c ascending). It starts
    // in the carry tile, so every step below sees "no dH_t" and no dH is allocated, zero-filled or read.
    for (int i = tid; i < FN; i += 1024) {
      const int f = i / N, n = i - f * N;
      T s = T(0);
      for (int c = 0; c < NC; ++c) s += dlogits[(size_t)b * NC + c] * head_w[(size_t)c * FN + i];
      carry[f * Ns + n] = s;
    }
    __syncthreads();
  }

  for (int t = Tn - 1; t >= 0; --t) {
    const T* xt = X + ((size_t)b * Tn + t) * GN;
    const T* hp = (t == 0) ? h0 + (size_t)b * FN : H + ((size_t)b * Tn + t - 1) * FN;
    const T* ht = H + ((size_t)b * Tn + t) * FN;
    const T* dht = dH ? dH + ((size_t)b * Tn + t) * FN : nullptr;
    const T* dyt = dY ? dY + ((size_t)b * Tn + t) * NC * N : nullptr;
    if (GATED && tid < 2 * N) {
      const int w = tid >= N, n = tid - w * N;
      gvec[w * Ns + n] = (w ? gf : gi)[b * gsb + t * gst + n * gsn];
    }
    for (int i = tid; i < (G + F) * N; i += 1024) {
      const int c = i / N, n = i - c * N;
      Z0[c * Ns + n] = (c < G) ? xt[i] : hp[i - GN];
    }
    for (int i = tid; i < FN; i += 1024) {
      const int f = i / N, n = i - f * N;
      const T h = ht[i];
      T d = dht ? dht[i] : T(0);
      if (dyt) {
        // per-node head upstream: dH_t[f][n] = sum_o node_w[o][f] dY[b][t][o][n] (o ascending) is formed here and never stored
        for (int o = 0; o < NC; ++o) d += head_w[(size_t)o * F + f] * dyt[o * N + n];
      }
      dpre[f * Ns + n] = (d + carry[f * Ns + n]) * (T(1) - h * h);
    }
    __syncthreads();
    // ---- levels k = 0 .. K-1: dW_k += dpre Z_k^T  |  (gated) ya / yb += W_k Z_k  |  Z_{k+1} = Z_k S
    acc_t ya[2], yb[2];
    if (GATED) { ya[0] = ya[1] = yb[0] = yb[1] = acc_t{0, 0, 0, 0}; }
    T* zc = Z0;
    T* zn = Z1;
    for (int k = 0; k < K; ++k) {
      // weight gradients of this level
#pragma unroll
      for (int q = 0; q < MAXW; ++q) {
        const int tile = wave + q * 16;
        if (tile < wtiles && tile / (tilesF * tilesC) == k) {
          const int rem = tile - k * (tilesF * tilesC);
          const int i0 = (rem / tilesC) << 4, j0 = (rem % tilesC) << 4;
          // A = dpre (i = f, k = n), B = Z_k^T (k = n, j = c): both "lanes over rows, lane groups over consecutive n"
          const T* ap = (i0 + li < F) ? dpre + (i0 + li) * Ns + lk : zrow + lk;
          const T* bp = (j0 + li < C) ? zc + (j0 + li) * Ns + lk : zrow + lk;
          // A = dpre (i = f, k = n), B = Z_k^T (k = n, j = c) scaled by the gate of (filter of column c, node n)
          if (GATED) wacc[q] = tile_mac_gated<T>(wacc[q], bp, gvec + ((j0 + li < G) ? 0 : Ns) + lk, ap, 4, N4 >> 2, true);
          else       wacc[q] = tile_mac<T>(wacc[q], ap, 4, bp, 4, N4 >> 2);
        }
      }
      if (GATED) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int tile = wave + q * 16;
          if (tile >= tilesF * tilesN) break;
          const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
          const T* wr = (i0 + li < F) ? WAl + ((size_t)(i0 + li) * K + k) * Cs : zrow;      // columns C .. Cs-1 are zero
          acc_t a = ya[q], bq = yb[q];
          const int G4 = (G + 3) & ~3;
          // x-columns c < G into ya, h-columns into yb (a k-step that straddles G contributes to both, masked by select)
          for (int c0 = 0; c0 < C4; c0 += 4) {
            const int c = c0 + lk;
            const T wv = wr[c];
            const T zv = zc[c * Ns + j0 + li];                       // rows C .. C4-1 are zero
            if (c0 < G4) a = Mf<T>::mma(c < G ? wv : T(0), zv, a);
            if (c0 + 3 >= G) bq = Mf<T>::mma(c >= G ? wv : T(0), zv, bq);
          }
          ya[q] = a; yb[q] = bq;
        }
      }
      if (k + 1 < K) {
        for (int tile = wave; tile < tilesC * tilesN; tile += 16) {
          const int tl = (tile + 5) % (tilesC * tilesN);          // start the hop tiles on other waves than the dW tiles
          const int i0 = (tl / tilesN) << 4, j0 = (tl % tilesN) << 4;
          acc_t acc = {0, 0, 0, 0};
          const T* ap = (i0 + li < C) ? zc + (i0 + li) * Ns + lk : zrow + lk;
          acc = tile_mac<T>(acc, ap, 4, S + lk * Ns + j0 + li, 4 * Ns, N4 >> 2);
          const int n = j0 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = i0 + Mf<T>::row(lane, r);
            if (c < C && n < N) zn[c * Ns + n] = acc[r];
          }
        }
        __syncthreads();
        T* tmp = zc; zc = zn; zn = tmp;
      }
    }
    __syncthreads();                    // the Z buffers are free: they become the adjoint accumulators
    // ---- bias / gate partial sums
    if (tid < F) {
      const T* dr = dpre + tid * Ns;
      T s = T(0);
      if (GATED) { for (int n = 0; n < N; ++n) s += dr[n] * (gvec[n] + gvec[Ns + n]); }
      else       { for (int n = 0; n < N; ++n) s += dr[n]; s *= T(2); }
      bacc += s;
    }
    if (GATED) {
      // d gate[n] = sum_f dpre[f][n] (filter output[f][n] + b[f]): each lane holds 4 rows of its column; the 4 lanes of a
      // column (lane, lane ^ 16, ^ 32, ^ 48) are folded by shuffles, the tilesF row tiles through LDS in a fixed order
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int tile = wave + q * 16;
        if (tile >= tilesF * tilesN) break;
        const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
        const int n = j0 + li;
        T si = T(0), sf = T(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = i0 + Mf<T>::row(lane, r);
          if (f < F && n < N) {
            const T bb = bias ? bias[f] : T(0);
            const T d = dpre[f * Ns + n];
            si += d * (ya[q][r] + bb);
            sf += d * (yb[q][r] + bb);
          }
        }
        si += __shfl_xor(si, 16, 64); si += __shfl_xor(si, 32, 64);
        sf += __shfl_xor(sf, 16, 64); sf += __shfl_xor(sf, 32, 64);
        if (n < N && lk == 0) {
          gpart[(i0 >> 4) * Ns + n] = si;
          gpart[(tilesF + (i0 >> 4)) * Ns + n] = sf;
        }
      }
      __syncthreads();
      if (tid < 2 * N) {
        const int w = tid >= N, n = tid - w * N;
        T a = T(0);
        for (int p = 0; p < tilesF; ++p) a += gpart[(w * tilesF + p) * Ns + n];
        (w ? dgf : dgi)[((size_t)b * Tn + t) * N + n] = a;
      }
    }
    // ---- carry_{t-1}: acc <- gf B_k^T dpre + acc S^T, k = Kst-1 .. 0
    T* ac = Z0;
    T* an = Z1;
    if (DX) {
      T* dxt = dX + ((size_t)b * Tn + t) * GN;
      for (int k = K - 1; k >= 0; --k) {
        const T* wk = WBt + (size_t)k * F4 * Cs1;
        for (int tile = wave; tile < tilesC * tilesN; tile += 16) {
          const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
          acc_t acc = {0, 0, 0, 0};
          // A = W_k^T (i = c, k = f) = wk[f][c] (masked rows read the zero column C), B = dpre (k = f, j = n)
          const bool arow = i0 + li < C;
          acc = tile_mac<T>(acc, wk + lk * Cs1 + (arow ? i0 + li : C), 4 * Cs1, dpre + lk * Ns + j0 + li, 4 * Ns, F4 >> 2);
          const int n = j0 + li;
          if (GATED) {
            const T gx = gvec[n < N ? n : 0], gh = gvec[Ns + (n < N ? n : 0)];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] *= (i0 + Mf<T>::row(lane, r) < G) ? gx : gh;
          }
          if (k < K - 1) {
            // A = acc (i = c, k = m), B = S^T (k = m, j = n) = S[n][m]
            const T* ap = arow ? ac + (i0 + li) * Ns + lk : zrow + lk;
            acc = tile_mac<T>(acc, ap, 4, S + (j0 + li) * Ns + lk, 4, N4 >> 2);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = i0 + Mf<T>::row(lane, r);
            if (c < C && n < N) {
              if (k > 0) an[c * Ns + n] = acc[r];
              else if (c < G) dxt[(size_t)c * N + n] = acc[r];
              else carry[(c - G) * Ns + n] = acc[r];
            }
          }
        }
        __syncthreads();
        T* tmp = ac; ac = an; an = tmp;
      }
    } else
    for (int k = Kst - 1; k >= 0; --k) {
      T* dst = (k == 0) ? carry : an;
      const T* wk = WBt + (size_t)k * F4 * Fs;
      for (int tile = wave; tile < tilesF * tilesN; tile += 16) {
        const int i0 = (tile / tilesN) << 4, j0 = (tile % tilesN) << 4;
        acc_t acc = {0, 0, 0, 0};
        // A = B_k^T (i = f2, k = f) = wk[f][f2], B = dpre (k = f, j = n)
        const bool acol = i0 + li < F;
        const int nb = j0 + li;
        acc = tile_mac<T>(acc, wk + lk * Fs + (acol ? i0 + li : F), 4 * Fs, dpre + lk * Ns + j0 + li, 4 * Ns, F4 >> 2, T(1),
                          GATED ? gvec[Ns + (nb < N ? nb : 0)] : T(1));
        if (k < Kst - 1) {
          // A = acc (i = f2, k = m), B = S^T (k = m, j = n) = S[n][m]
          const T* ap = acol ? ac + (i0 + li) * Ns + lk : zrow + lk;
          acc = tile_mac<T>(acc, ap, 4, S + (j0 + li) * Ns + lk, 4, N4 >> 2);
        }
        const int n = j0 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f2 = i0 + Mf<T>::row(lane, r);
          if (f2 < F && n < N) dst[f2 * Ns + n] = acc[r];
        }
      }
      __syncthreads();
      T* tmp = ac; ac = an; an = tmp;
    }
  }

  // ---- results
  if (dh0)
    for (int i = tid; i < FN; i += 1024) {
      const int f = i / N, n = i - f * N;
      dh0[(size_t)b * FN + i] = carry[f * Ns + n];
    }
  if (tid < F) pb[(size_t)b * F + tid] = bacc;
#pragma unroll
  for (int q = 0; q < MAXW; ++q) {
    const int tile = wave + q * 16;
    if (tile < wtiles) {
      const int k = tile / (tilesF * tilesC), rem = tile - k * (tilesF * tilesC);
      const int i0 = (rem / tilesC) << 4, j0 = (rem % tilesC) << 4;
      const int c = j0 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = i0 + Mf<T>::row(lane, r);
        if (f < F && c < C) {
          if (c < G) { if (k < Kin) pA[(((size_t)b * F + f) * Kin + k) * G + c] = wacc[q][r]; }
          else       { if (k < Kst) pB[(((size_t)b * F + f) * Kst + k) * F + (c - G)] = wacc[q][r]; }
        }
      }
    }
  }
}

template <typename T>
size_t dense_bwd_lds(int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, bool gated, bool dx = false) {
  const int K = (int)(Kin > Kst ? Kin : Kst), C = (int)(G + F);
  const int Ns = lds_stride<T>((int)N), Fs = lds_stride<T>((int)F + 1), Cs = lds_stride<T>(C), Cs1 = lds_stride<T>(C + 1);
  const int F4 = ((int)F + 3) & ~3, C4 = (C + 3) & ~3;
  const int SR = (((int)N + 15) >> 4) * 16;
  return sizeof(T) * ((size_t)SR * Ns + 2 * (size_t)C4 * Ns + 2 * (size_t)F4 * Ns +
                      (dx ? (size_t)K * F4 * Cs1 : (size_t)Kst * F4 * Fs) +
                      (gated ? (size_t)F * K * Cs : 0) + 64 + (size_t)(Ns > K * Cs ? Ns : K * Cs) +
                      (gated ? (2 + 2 * (size_t)(((int)F + 15) >> 4)) * Ns : 0)) + 16;
}

// what the per-node head adds to the forward image: node_w [O][F] with node_b in a column of its own (the backward reads node_w from
// global memory: one value per element and step, next to the dY it multiplies)
template <typename T>
size_t dense_node_head_lds(int64_t F, int64_t O) { return sizeof(T) * (size_t)O * (size_t)(F + 1); }

// what the graph-filter head adds to the forward image: head_w [K_o][F] and the bias (rounded up to four values), and the state rows
// [F4][Ns] of each hop level the cell does not compute itself (K_o > K)
template <typename T>
size_t dense_gnn_head_lds(int64_t N, int64_t F, int64_t K, int64_t Ko) {
  const size_t F4 = (size_t)((F + 3) & ~(int64_t)3), Ns = (size_t)lds_stride<T>((int)N);
  return sizeof(T) * ((size_t)((Ko * F + 1 + 3) & ~(int64_t)3) + (Ko > K ? (size_t)(Ko - K) * F4 * Ns : 0));
}

// the graph-filter head followed by a read-out on the last state: the graph-filter head's share and its output vector v [Ns]
template <typename T>
size_t dense_cls_gnn_head_lds(int64_t N, int64_t F, int64_t K, int64_t Ko) {
  return dense_gnn_head_lds<T>(N, F, K, Ko) + sizeof(T) * (size_t)lds_stride<T>((int)N);
}

constexpr size_t DENSE_LDS_MAX = 160 * 1024;

template <typename T>
bool dense_shape_ok(int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst) {
  if (N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0 || N > 256 || F > 256 || G > 256 || Kin > 8 || Kst > 8) return false;
  return true;
}

}  // namespace

extern "C" int gcrnn_small_dense_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst,
                                           int backward, int gated) {
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return 0;
  const int64_t K = Kin > Kst ? Kin : Kst;
  const int64_t tilesN = (N + 15) / 16, tilesF = (F + 15) / 16, tilesC = (G + F + 15) / 16;
  if (dtype == GCRNN_F32) {
    if (!dense_shape_ok<float>(N, G, F, Kin, Kst)) return 0;
    if (!backward) return tilesF * tilesN <= 16 * 4 && dense_fwd_lds<float>(N, G, F, K) <= DENSE_LDS_MAX;
    return K * tilesF * tilesC <= 16 * 4 && (!gated || tilesF * tilesN <= 32) &&
           dense_bwd_lds<float>(N, G, F, Kin, Kst, gated != 0) <= DENSE_LDS_MAX;
  }
  if (!dense_shape_ok<double>(N, G, F, Kin, Kst)) return 0;
  if (!backward) return tilesF * tilesN <= 16 * 4 && dense_fwd_lds<double>(N, G, F, K) <= DENSE_LDS_MAX;
  return K * tilesF * tilesC <= 16 * 4 && (!gated || tilesF * tilesN <= 32) &&
         dense_bwd_lds<double>(N, G, F, Kin, Kst, gated != 0) <= DENSE_LDS_MAX;
}

// The backward pass with dX: the predicate of the plain backward, with the LDS image of the DX variant.
extern "C" int gcrnn_small_dense_backward_dx_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst,
                                                       int gated) {
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, 1, gated)) return 0;
  const size_t lds = dtype == GCRNN_F32 ? dense_bwd_lds<float>(N, G, F, Kin, Kst, gated != 0, true)
                                        : dense_bwd_lds<double>(N, G, F, Kin, Kst, gated != 0, true);
  return lds <= DENSE_LDS_MAX ? 1 : 0;
}

// One forward launch, filled by field name at each entry. The head: the read-out head_w [NC][F N], head_b [NC], out = logits [B][NC]
// (FWD_LAST), or node_w [NC][F], node_b [NC], out = Y [B][T][NC][N] (FWD_NODE).
struct DenseFwdArgs {
  const void *X, *h0, *wA, *wB, *bias, *gi, *gf, *Sd;
  void* H;
  int64_t B, T, N, G, F, Kin, Kst, gsb, gst, gsn;
  hipStream_t st;
  const void *head_w = nullptr, *head_b = nullptr;
  void* out = nullptr;
  int64_t NC = 0;
  int store = GCRNN_SMALL_STATES_ALL;
  int act = 0;                     // FWD_GNN: head_w [NC][F] the head's taps, head_b [1], out = Y [B][T][1][N], NC = K_o
  const void *lin_w = nullptr, *lin_b = nullptr;      // FWD_CLS_GNN: FWD_GNN's head on the last state, then lin_w [NL][N], lin_b [NL];
  void* V = nullptr;                                  // out = logits [B][NL], V [B][N] the head's output or null
  int64_t NL = 0;
};

// One BPTT launch. The upstream gradient: dH [B][T][F][N]; or dlogits [B][NC] with head_w [NC][F N] (read-out on the last state); or
// dY [B][T][NC][N] with head_w = node_w [NC][F] (per-node head); or dU (below). dX == nullptr selects the plain variant.
struct DenseBwdArgs {
  const void *X, *h0, *H, *wA, *wB, *bias, *gi, *gf, *Sd;
  void *pA, *pB, *pb, *dgi, *dgf, *dh0, *dX;
  int64_t B, T, N, G, F, Kin, Kst, gsb, gst, gsn;
  hipStream_t st;
  const void *dH = nullptr, *dlogits = nullptr, *dY = nullptr, *head_w = nullptr;
  int64_t NC = 0;
  void* dU = nullptr;              // graph-filter head + read-out on the last state: dlogits [B][NC], lin_w [NC][N], V [B][N], head_w
  const void *lin_w = nullptr, *V = nullptr;      // [Ko][F] the head's taps, dU [B][Ko][N] written by the launch
  int64_t Ko = 0;
  int act = 0;
};

// What the entries share, in the order they ask it: a gate comes with its partner and, in a backward pass (want_dg), with room for both
// gate gradients; the dtype where the entry answers for it itself (own_dtype: all but gcrnn_small_dense_forward / _backward, which leave it
// to the support query and so answer UNSUPPORTED). Then B and T positive, B a grid size: apart, two entries check their store mode first.
static int dense_shared_status(const void* gi, const void* gf, bool want_dg, const void* dgi, const void* dgf, bool own_dtype, int dtype) {
  if ((gi == nullptr) != (gf == nullptr) || (want_dg && gi && (!dgi || !dgf))) return GCRNN_ERR_NULL_POINTER;
  return own_dtype && dtype != GCRNN_F32 && dtype != GCRNN_F64 ? GCRNN_ERR_BAD_DTYPE : GCRNN_OK;
}
static bool dense_bt_ok(int64_t B, int64_t T) { return B > 0 && T > 0 && B <= 2147483647LL; }

template <typename T>
static int dense_fwd_launch(const DenseFwdArgs& a, int mode) {
  const int64_t N = a.N, F = a.F, K = a.Kin > a.Kst ? a.Kin : a.Kst;
  const size_t lds = dense_fwd_lds<T>(N, a.G, F, K) + (mode == FWD_NODE ? dense_node_head_lds<T>(F, a.NC) : 0) +
                     (mode == FWD_GNN ? dense_gnn_head_lds<T>(N, F, K, a.NC) : 0) +
                     (mode == FWD_CLS_GNN ? dense_cls_gnn_head_lds<T>(N, F, K, a.NC) : 0);
  const int64_t ot = ((F + 15) / 16) * ((N + 15) / 16);             // output tiles per step, dealt over 16 waves
  auto kern = mode == FWD_CLS_GNN ? (ot <= 16 ? small_dense_fwd_kernel<T, 1, FWD_CLS_GNN> : (ot <= 32 ? small_dense_fwd_kernel<T, 2, FWD_CLS_GNN> : small_dense_fwd_kernel<T, 4, FWD_CLS_GNN>))
              : mode == FWD_GNN ? (ot <= 16 ? small_dense_fwd_kernel<T, 1, FWD_GNN> : (ot <= 32 ? small_dense_fwd_kernel<T, 2, FWD_GNN> : small_dense_fwd_kernel<T, 4, FWD_GNN>))
              : mode == FWD_NODE ? (ot <= 16 ? small_dense_fwd_kernel<T, 1, FWD_NODE> : (ot <= 32 ? small_dense_fwd_kernel<T, 2, FWD_NODE> : small_dense_fwd_kernel<T, 4, FWD_NODE>))
              : mode == FWD_LAST ? (ot <= 16 ? small_dense_fwd_kernel<T, 1, FWD_LAST> : (ot <= 32 ? small_dense_fwd_kernel<T, 2, FWD_LAST> : small_dense_fwd_kernel<T, 4, FWD_LAST>))
                                 : (ot <= 16 ? small_dense_fwd_kernel<T, 1, FWD_PLAIN> : (ot <= 32 ? small_dense_fwd_kernel<T, 2, FWD_PLAIN> : small_dense_fwd_kernel<T, 4, FWD_PLAIN>));
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kern<<<(unsigned)a.B, 1024, lds, a.st>>>((const T*)a.X, (const T*)a.h0, (const T*)a.wA, (const T*)a.wB, (const T*)a.bias, (const T*)a.gi,
                                          (const T*)a.gf, (const T*)a.Sd, (T*)a.H, (int)a.T, (int)N, (int)a.G, (int)F, (int)a.Kin, (int)a.Kst,
                                          (int)a.B, a.gsb, a.gst, a.gsn, (const T*)a.head_w, (const T*)a.head_b, (T*)a.out, (int)a.NC, a.store, a.act,
                                          (const T*)a.lin_w, (const T*)a.lin_b, (T*)a.V, (int)a.NL);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// The one place that picks the forward instantiation: <T> here, MAXT and the mode (FWD_PLAIN / FWD_LAST / FWD_NODE / FWD_GNN / FWD_CLS_GNN) in the launcher.
static int dense_fwd_run(int dtype, const DenseFwdArgs& a, int mode) {
  return dtype == GCRNN_F32 ? dense_fwd_launch<float>(a, mode) : dense_fwd_launch<double>(a, mode);
}

extern "C" int gcrnn_small_dense_forward(int dtype, const void* X, const void* h0, const void* wA, const void* wB,
                                         const void* bias, const void* gi, const void* gf, const void* Sdense, void* H,
                                         int64_t B, int64_t T, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst,
                                         int64_t gate_stride_b, int64_t gate_stride_t, int64_t gate_stride_n, void* stream) {
  if (!X || !h0 || !wA || !wB || !Sdense || !H) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, false, nullptr, nullptr, false, dtype)) return s;
  if (!dense_bt_ok(B, T)) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, 0, gi != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseFwdArgs a{.X = X, .h0 = h0, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .H = H, .B = B, .T = T, .N = N,
                       .G = G, .F = F, .Kin = Kin, .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n,
                       .st = as_stream(stream)};
  return dense_fwd_run(dtype, a, FWD_PLAIN);
}

template <typename T, bool GATED, bool DX>
static int dense_bwd_launch(const DenseBwdArgs& a) {
  const int64_t N = a.N, G = a.G, F = a.F, Kin = a.Kin, Kst = a.Kst;
  const size_t lds = dense_bwd_lds<T>(N, G, F, Kin, Kst, GATED, DX);
  const int64_t wt = (Kin > Kst ? Kin : Kst) * ((F + 15) / 16) * ((G + F + 15) / 16);   // weight-gradient tiles, persistent
  auto kern = wt <= 16 ? small_dense_bwd_kernel<T, GATED, 1, DX>
                       : (wt <= 32 ? small_dense_bwd_kernel<T, GATED, 2, DX> : small_dense_bwd_kernel<T, GATED, 4, DX>);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kern<<<(unsigned)a.B, 1024, lds, a.st>>>((const T*)a.X, (const T*)a.h0, (const T*)a.H, (const T*)a.dH, (const T*)a.wA, (const T*)a.wB,
                                          (const T*)a.bias, (const T*)a.gi, (const T*)a.gf, (const T*)a.Sd, (T*)a.pA, (T*)a.pB, (T*)a.pb,
                                          (T*)a.dgi, (T*)a.dgf, (T*)a.dh0, (T*)a.dX, (int)a.T, (int)N, (int)G, (int)F, (int)Kin, (int)Kst,
                                          (int)a.B, a.gsb, a.gst, a.gsn, (const T*)a.dlogits, (const T*)a.head_w, (int)a.NC, (const T*)a.dY,
                                          (T*)a.dU, (const T*)a.lin_w, (const T*)a.V, (int)a.Ko, a.act);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

// The one place that picks the BPTT instantiation: <T, GATED, DX> from the dtype, gi != nullptr and dX != nullptr here, MAXW in the launcher.
static int dense_bwd_run(int dtype, const DenseBwdArgs& a) {
  const bool f32 = dtype == GCRNN_F32, gated = a.gi != nullptr;
  if (!a.dX) {
    if (f32) return gated ? dense_bwd_launch<float, true, false>(a) : dense_bwd_launch<float, false, false>(a);
    return gated ? dense_bwd_launch<double, true, false>(a) : dense_bwd_launch<double, false, false>(a);
  }
  if (f32) return gated ? dense_bwd_launch<float, true, true>(a) : dense_bwd_launch<float, false, true>(a);
  return gated ? dense_bwd_launch<double, true, true>(a) : dense_bwd_launch<double, false, true>(a);
}

extern "C" int gcrnn_small_dense_backward(int dtype, const void* X, const void* h0, const void* H, const void* dH,
                                          const void* wA, const void* wB, const void* bias, const void* gi, const void* gf,
                                          const void* Sdense, void* pA, void* pB, void* pb, void* dgi, void* dgf, void* dh0,
                                          int64_t B, int64_t T, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst,
                                          int64_t gate_stride_b, int64_t gate_stride_t, int64_t gate_stride_n, void* stream) {
  if (!X || !h0 || !H || !dH || !wA || !wB || !Sdense || !pA || !pB || !pb) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, true, dgi, dgf, false, dtype)) return s;
  if (!dense_bt_ok(B, T)) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, 1, gi != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseBwdArgs a{.X = X, .h0 = h0, .H = H, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .pA = pA, .pB = pB,
                       .pb = pb, .dgi = dgi, .dgf = dgf, .dh0 = dh0, .dX = nullptr, .B = B, .T = T, .N = N, .G = G, .F = F, .Kin = Kin,
                       .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n, .st = as_stream(stream), .dH = dH};
  return dense_bwd_run(dtype, a);
}

extern "C" int gcrnn_small_dense_backward_dx(int dtype, const void* X, const void* h0, const void* H, const void* dH,
                                             const void* wA, const void* wB, const void* bias, const void* gi, const void* gf,
                                             const void* Sdense, void* pA, void* pB, void* pb, void* dgi, void* dgf, void* dh0,
                                             void* dX, int64_t B, int64_t T, int64_t N, int64_t G, int64_t F, int64_t Kin,
                                             int64_t Kst, int64_t gate_stride_b, int64_t gate_stride_t, int64_t gate_stride_n,
                                             void* stream) {
  if (!X || !h0 || !H || !dH || !wA || !wB || !Sdense || !pA || !pB || !pb || !dX) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, true, dgi, dgf, true, dtype)) return s;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_backward_dx_supported(dtype, N, G, F, Kin, Kst, gi != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseBwdArgs a{.X = X, .h0 = h0, .H = H, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .pA = pA, .pB = pB,
                       .pb = pb, .dgi = dgi, .dgf = dgf, .dh0 = dh0, .dX = dX, .B = B, .T = T, .N = N, .G = G, .F = F, .Kin = Kin,
                       .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n, .st = as_stream(stream), .dH = dH};
  return dense_bwd_run(dtype, a);
}

// ------------------------------------------------------------------------------------------------------------------
// read-out on the last state (the classification model): logits from the forward launch, BPTT seeded from dlogits
// ------------------------------------------------------------------------------------------------------------------
extern "C" int gcrnn_small_dense_head_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t C,
                                                int backward, int gated, int dx) {
  if (C <= 0 || C > GCRNN_SMALL_HEAD_MAX_CLASSES) return 0;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, backward, gated)) return 0;
  if (dx && !gcrnn_small_dense_backward_dx_supported(dtype, N, G, F, Kin, Kst, gated)) return 0;
  return 1;
}

extern "C" int gcrnn_small_dense_forward_head(int dtype, const void* X, const void* h0, const void* wA, const void* wB,
                                              const void* bias, const void* gi, const void* gf, const void* Sdense,
                                              const void* head_w, const void* head_b, void* H, void* logits, int64_t B, int64_t T,
                                              int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b,
                                              int64_t gate_stride_t, int64_t gate_stride_n, int64_t C, int store_states,
                                              void* stream) {
  if (!X || !h0 || !wA || !wB || !Sdense) return GCRNN_ERR_NULL_POINTER;
  if ((head_w == nullptr) != (logits == nullptr) || (!head_w && head_b)) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, false, nullptr, nullptr, true, dtype)) return s;
  if (store_states != GCRNN_SMALL_STATES_ALL && store_states != GCRNN_SMALL_STATES_LAST && store_states != GCRNN_SMALL_STATES_NONE)
    return GCRNN_ERR_BAD_SHAPE;
  if (store_states == GCRNN_SMALL_STATES_NONE ? !head_w : !H) return GCRNN_ERR_NULL_POINTER;      // a launch with nothing to write / no H
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (head_w ? C <= 0 : C != 0) return GCRNN_ERR_BAD_SHAPE;
  if (head_w ? !gcrnn_small_dense_head_supported(dtype, N, G, F, Kin, Kst, C, 0, gi != nullptr, 0)
             : !gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, 0, gi != nullptr))
    return GCRNN_ERR_UNSUPPORTED;
  const DenseFwdArgs a{.X = X, .h0 = h0, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .H = H, .B = B, .T = T, .N = N,
                       .G = G, .F = F, .Kin = Kin, .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n,
                       .st = as_stream(stream), .head_w = head_w, .head_b = head_b, .out = logits, .NC = C, .store = store_states};
  return dense_fwd_run(dtype, a, head_w || store_states != GCRNN_SMALL_STATES_ALL ? FWD_LAST : FWD_PLAIN);   // else the plain recurrence
}

extern "C" int gcrnn_small_dense_backward_head(int dtype, const void* X, const void* h0, const void* H, const void* dlogits,
                                               const void* head_w, const void* wA, const void* wB, const void* bias,
                                               const void* gi, const void* gf, const void* Sdense, void* pA, void* pB, void* pb,
                                               void* dgi, void* dgf, void* dh0, void* dX, int64_t B, int64_t T, int64_t N,
                                               int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b,
                                               int64_t gate_stride_t, int64_t gate_stride_n, int64_t C, void* stream) {
  if (!X || !h0 || !H || !dlogits || !head_w || !wA || !wB || !Sdense || !pA || !pB || !pb) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, true, dgi, dgf, true, dtype)) return s;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0 || C <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_head_supported(dtype, N, G, F, Kin, Kst, C, 1, gi != nullptr, dX != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseBwdArgs a{.X = X, .h0 = h0, .H = H, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .pA = pA, .pB = pB,
                       .pb = pb, .dgi = dgi, .dgf = dgf, .dh0 = dh0, .dX = dX, .B = B, .T = T, .N = N, .G = G, .F = F, .Kin = Kin,
                       .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n, .st = as_stream(stream),
                       .dlogits = dlogits, .head_w = head_w, .NC = C};
  return dense_bwd_run(dtype, a);
}

// ------------------------------------------------------------------------------------------------------------------
// per-node head on every state (the regression model's `multipMlp` head): Y from the forward launch, BPTT fed dY and node_w
// ------------------------------------------------------------------------------------------------------------------
extern "C" int gcrnn_small_dense_node_head_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t O,
                                                     int backward, int gated, int dx) {
  if (O <= 0 || O > GCRNN_SMALL_NODE_HEAD_MAX_OUT) return 0;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, backward, gated)) return 0;
  if (dx && !gcrnn_small_dense_backward_dx_supported(dtype, N, G, F, Kin, Kst, gated)) return 0;
  if (backward) return 1;               // the backward reads node_w from global memory: the LDS image of the plain backward
  const int64_t K = Kin > Kst ? Kin : Kst;
  const size_t lds = dtype == GCRNN_F32 ? dense_fwd_lds<float>(N, G, F, K) + dense_node_head_lds<float>(F, O)
                                        : dense_fwd_lds<double>(N, G, F, K) + dense_node_head_lds<double>(F, O);
  return lds <= DENSE_LDS_MAX ? 1 : 0;
}

extern "C" int gcrnn_small_dense_forward_node_head(int dtype, const void* X, const void* h0, const void* wA, const void* wB,
                                                   const void* bias, const void* gi, const void* gf, const void* Sdense,
                                                   const void* node_w, const void* node_b, void* H, void* Y, int64_t B, int64_t T,
                                                   int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b,
                                                   int64_t gate_stride_t, int64_t gate_stride_n, int64_t O, int store_states,
                                                   void* stream) {
  if (!X || !h0 || !wA || !wB || !Sdense || !node_w || !Y) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, false, nullptr, nullptr, true, dtype)) return s;
  if (store_states != GCRNN_SMALL_STATES_ALL && store_states != GCRNN_SMALL_STATES_LAST && store_states != GCRNN_SMALL_STATES_NONE)
    return GCRNN_ERR_BAD_SHAPE;
  if (store_states != GCRNN_SMALL_STATES_NONE && !H) return GCRNN_ERR_NULL_POINTER;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (O <= 0 || O > GCRNN_SMALL_NODE_HEAD_MAX_OUT) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_node_head_supported(dtype, N, G, F, Kin, Kst, O, 0, gi != nullptr, 0)) return GCRNN_ERR_UNSUPPORTED;
  // the training forward stores the states of the forward-only image; its backward is asked separately
  const DenseFwdArgs a{.X = X, .h0 = h0, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .H = H, .B = B, .T = T, .N = N,
                       .G = G, .F = F, .Kin = Kin, .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n,
                       .st = as_stream(stream), .head_w = node_w, .head_b = node_b, .out = Y, .NC = O, .store = store_states};
  return dense_fwd_run(dtype, a, FWD_NODE);
}

extern "C" int gcrnn_small_dense_backward_node_head(int dtype, const void* X, const void* h0, const void* H, const void* dY,
                                                    const void* node_w, const void* wA, const void* wB, const void* bias,
                                                    const void* gi, const void* gf, const void* Sdense, void* pA, void* pB, void* pb,
                                                    void* dgi, void* dgf, void* dh0, void* dX, int64_t B, int64_t T, int64_t N,
                                                    int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b,
                                                    int64_t gate_stride_t, int64_t gate_stride_n, int64_t O, void* stream) {
  if (!X || !h0 || !H || !dY || !node_w || !wA || !wB || !Sdense || !pA || !pB || !pb) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, true, dgi, dgf, true, dtype)) return s;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (O <= 0 || O > GCRNN_SMALL_NODE_HEAD_MAX_OUT) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_node_head_supported(dtype, N, G, F, Kin, Kst, O, 1, gi != nullptr, dX != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseBwdArgs a{.X = X, .h0 = h0, .H = H, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .pA = pA, .pB = pB,
                       .pb = pb, .dgi = dgi, .dgf = dgf, .dh0 = dh0, .dX = dX, .B = B, .T = T, .N = N, .G = G, .F = F, .Kin = Kin,
                       .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n, .st = as_stream(stream), .dY = dY,
                       .head_w = node_w, .NC = O};
  return dense_bwd_run(dtype, a);
}

// ------------------------------------------------------------------------------------------------------------------
// one-layer graph-filter head on every state (the regression model's Selection-GNN head, GraphFilter(F -> 1, K_o) + activation): Y from
// the forward launch; the backward is gcrnn_small_gnn_head_adjoint (gcrnn_small_gnn_head.hip) + gcrnn_small_dense_backward_node_head
// ------------------------------------------------------------------------------------------------------------------
extern "C" int gcrnn_small_dense_gnn_head_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t Ko,
                                                    int backward, int gated, int dx) {
  if (Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT) return 0;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, backward, gated)) return 0;
  if (backward) {
    // the BPTT launch takes the head's share as a per-node head of O = K_o outputs; the adjoint kernel's own image is S and eight rows
    if (!gcrnn_small_dense_node_head_supported(dtype, N, G, F, Kin, Kst, Ko, 1, gated, dx)) return 0;
    return (dtype == GCRNN_F32 ? gnn_adjoint_lds<float>(N) : gnn_adjoint_lds<double>(N)) <= DENSE_LDS_MAX ? 1 : 0;
  }
  const int64_t K = Kin > Kst ? Kin : Kst;
  const size_t lds = dtype == GCRNN_F32 ? dense_fwd_lds<float>(N, G, F, K) + dense_gnn_head_lds<float>(N, F, K, Ko)
                                        : dense_fwd_lds<double>(N, G, F, K) + dense_gnn_head_lds<double>(N, F, K, Ko);
  return lds <= DENSE_LDS_MAX ? 1 : 0;
}

extern "C" int gcrnn_small_dense_forward_gnn_head(int dtype, const void* X, const void* h0, const void* wA, const void* wB,
                                                  const void* bias, const void* gi, const void* gf, const void* Sdense,
                                                  const void* head_w, const void* head_b, void* H, void* Y, int64_t B, int64_t T,
                                                  int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b,
                                                  int64_t gate_stride_t, int64_t gate_stride_n, int64_t Ko, int act, int store_states,
                                                  void* stream) {
  if (!X || !h0 || !wA || !wB || !Sdense || !head_w || !Y) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, false, nullptr, nullptr, true, dtype)) return s;
  if (store_states != GCRNN_SMALL_STATES_ALL && store_states != GCRNN_SMALL_STATES_LAST && store_states != GCRNN_SMALL_STATES_NONE)
    return GCRNN_ERR_BAD_SHAPE;
  if (store_states != GCRNN_SMALL_STATES_NONE && !H) return GCRNN_ERR_NULL_POINTER;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT || act < 0 || act > 3) return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_gnn_head_supported(dtype, N, G, F, Kin, Kst, Ko, 0, gi != nullptr, 0)) return GCRNN_ERR_UNSUPPORTED;
  const DenseFwdArgs a{.X = X, .h0 = h0, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .H = H, .B = B, .T = T, .N = N,
                       .G = G, .F = F, .Kin = Kin, .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n,
                       .st = as_stream(stream), .head_w = head_w, .head_b = head_b, .out = Y, .NC = Ko, .store = store_states, .act = act};
  return dense_fwd_run(dtype, a, FWD_GNN);
}

// ------------------------------------------------------------------------------------------------------------------
// one-layer graph-filter head + read-out Linear(N -> C) on the LAST state (the classification model's Selection-GNN head, GraphFilter(F -> 1,
// K_o) + activation, then nn.Linear): logits from the forward launch (FWD_CLS_GNN), BPTT seeded from dlogits inside its launch, which also
// writes the head's adjoint levels dU [B][K_o][N] for the parameter gradients
// ------------------------------------------------------------------------------------------------------------------
extern "C" int gcrnn_small_dense_cls_gnn_head_supported(int dtype, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t Ko,
                                                        int64_t C, int backward, int gated, int dx) {
  if (Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT || C <= 0 || C > GCRNN_SMALL_HEAD_MAX_CLASSES) return 0;
  if (!gcrnn_small_dense_supported(dtype, N, G, F, Kin, Kst, backward, gated)) return 0;
  if (dx && !gcrnn_small_dense_backward_dx_supported(dtype, N, G, F, Kin, Kst, gated)) return 0;
  if (backward) return 1;               // the seeding borrows two rows of the BPTT launch's own Z tile: the LDS image of the plain backward
  const int64_t K = Kin > Kst ? Kin : Kst;
  const size_t lds = dtype == GCRNN_F32 ? dense_fwd_lds<float>(N, G, F, K) + dense_cls_gnn_head_lds<float>(N, F, K, Ko)
                                        : dense_fwd_lds<double>(N, G, F, K) + dense_cls_gnn_head_lds<double>(N, F, K, Ko);
  return lds <= DENSE_LDS_MAX ? 1 : 0;
}

extern "C" int gcrnn_small_dense_forward_cls_gnn_head(int dtype, const void* X, const void* h0, const void* wA, const void* wB,
                                                      const void* bias, const void* gi, const void* gf, const void* Sdense,
                                                      const void* head_w, const void* head_b, const void* lin_w, const void* lin_b,
                                                      void* H, void* V, void* logits, int64_t B, int64_t T, int64_t N, int64_t G,
                                                      int64_t F, int64_t Kin, int64_t Kst, int64_t gate_stride_b, int64_t gate_stride_t,
                                                      int64_t gate_stride_n, int64_t Ko, int64_t C, int act, int store_states,
                                                      void* stream) {
  if (!X || !h0 || !wA || !wB || !Sdense || !head_w || !lin_w || !logits) return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, false, nullptr, nullptr, true, dtype)) return s;
  if (store_states != GCRNN_SMALL_STATES_ALL && store_states != GCRNN_SMALL_STATES_LAST && store_states != GCRNN_SMALL_STATES_NONE)
    return GCRNN_ERR_BAD_SHAPE;
  if (store_states != GCRNN_SMALL_STATES_NONE && !H) return GCRNN_ERR_NULL_POINTER;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT || C <= 0 || C > GCRNN_SMALL_HEAD_MAX_CLASSES || act < 0 || act > 3)
    return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_cls_gnn_head_supported(dtype, N, G, F, Kin, Kst, Ko, C, 0, gi != nullptr, 0)) return GCRNN_ERR_UNSUPPORTED;
  // the training forward stores the states of the forward-only image; its backward is asked separately
  const DenseFwdArgs a{.X = X, .h0 = h0, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .H = H, .B = B, .T = T, .N = N,
                       .G = G, .F = F, .Kin = Kin, .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n,
                       .st = as_stream(stream), .head_w = head_w, .head_b = head_b, .out = logits, .NC = Ko, .store = store_states, .act = act,
                       .lin_w = lin_w, .lin_b = lin_b, .V = V, .NL = C};
  return dense_fwd_run(dtype, a, FWD_CLS_GNN);
}

extern "C" int gcrnn_small_dense_backward_cls_gnn_head(int dtype, const void* X, const void* h0, const void* H, const void* dlogits,
                                                       const void* lin_w, const void* V, const void* head_w, const void* wA,
                                                       const void* wB, const void* bias, const void* gi, const void* gf,
                                                       const void* Sdense, void* pA, void* pB, void* pb, void* dgi, void* dgf, void* dh0,
                                                       void* dX, void* dU, int64_t B, int64_t T, int64_t N, int64_t G, int64_t F,
                                                       int64_t Kin, int64_t Kst, int64_t gate_stride_b, int64_t gate_stride_t,
                                                       int64_t gate_stride_n, int64_t Ko, int64_t C, int act, void* stream) {
  if (!X || !h0 || !H || !dlogits || !lin_w || !V || !head_w || !wA || !wB || !Sdense || !pA || !pB || !pb || !dU)
    return GCRNN_ERR_NULL_POINTER;
  if (int s = dense_shared_status(gi, gf, true, dgi, dgf, true, dtype)) return s;
  if (!dense_bt_ok(B, T) || N <= 0 || G <= 0 || F <= 0 || Kin <= 0 || Kst <= 0) return GCRNN_ERR_BAD_SHAPE;
  if (Ko <= 0 || Ko > GCRNN_SMALL_NODE_HEAD_MAX_OUT || C <= 0 || C > GCRNN_SMALL_HEAD_MAX_CLASSES || act < 0 || act > 3)
    return GCRNN_ERR_BAD_SHAPE;
  if (!gcrnn_small_dense_cls_gnn_head_supported(dtype, N, G, F, Kin, Kst, Ko, C, 1, gi != nullptr, dX != nullptr)) return GCRNN_ERR_UNSUPPORTED;
  const DenseBwdArgs a{.X = X, .h0 = h0, .H = H, .wA = wA, .wB = wB, .bias = bias, .gi = gi, .gf = gf, .Sd = Sdense, .pA = pA, .pB = pB,
                       .pb = pb, .dgi = dgi, .dgf = dgf, .dh0 = dh0, .dX = dX, .B = B, .T = T, .N = N, .G = G, .F = F, .Kin = Kin,
                       .Kst = Kst, .gsb = gate_stride_b, .gst = gate_stride_t, .gsn = gate_stride_n, .st = as_stream(stream),
                       .dlogits = dlogits, .head_w = head_w, .NC = C, .dU = dU, .lin_w = lin_w, .V = V, .Ko = Ko, .act = act};
  return dense_bwd_run(dtype, a);
}
