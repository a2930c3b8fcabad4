// Small-graph regime, EDGE-gated cell (spatial_gating = 'edge', optionally time-gated too), training: BPTT of the recurrence that
// small_edge_cell_kernel (gcrnn_small_edge.hip; notation of its header comment) runs forward. Only H is kept by the forward; every
// step's intermediates are recomputed here from h_{t-1} (state branch) or x_t (input branch).
//
// XP = false, one workgroup per sequence, t = T-1 .. 0 with the carried dh in LDS:
//   recompute z_k, Wx | s1 | s2, mx, den, coef, acc from h_{t-1}
//   dpre = (dH_t + dh) (1 - h_t^2)  -> scratch dPre[b][t] (the input branch's upstream),  dgf[t][b] = sum dpre relu(acc)
//   dy = gf_t dpre [acc > 0]
//   column pass^T:   p[q] = coef[q] sum_f dy[f][n_q] Wx[f][m_q]  (= alpha dalpha),   dWx[f][m] = sum_{q in row m} coef[q] dy[f][n_q]
//   softmax^T:       de[q] = p[q] - alpha[q] sum_{row m_q} p,  dzz = de (zz > 0 ? 1 : 0.2: the slope at 0 is the negative one, as torch leaky_relu has it),  ds1[n] = sum_{column n} dzz,  ds2[m] = sum_{row m} dzz
//   folded taps^T:   dwf[r][k][c] += sum_n dwx[r][n] z_k[c][n],  dbf[r] += sum_n dwx[r][n]   (dwx = dWx | ds1 | ds2; registers, all t)
//   hops^T (Horner): g_{K-1} = dz_{K-1},  g_{k-1} = dz_{k-1} + g_k S^T  with  dz_k[c][n] = sum_r wf[r][k][c] dwx[r][n];  dh <- g_0
// XP = true, one workgroup per (b, t): the same from x_t with dPre[b][t] as upstream and the gate gi. Without DX it ends at the folded
//   taps' adjoint (no gradient for X). With DX (XP only) the hops' adjoint runs here too, on the C = G channels with K = Kin, and its
//   g_0 is dX[b][t]; gi_t is already inside dy, so nothing more is scaled. K = 1 has no hop: dX = dz_0.
// Row-ordered sums walk the support rows through `inv`, the inverse of the permutation t_pos (row position of column-ordered edge q).
// The gradients of the FOLDED taps and bias leave in per-workgroup slots; the host side sums the slots and unfolds them.
// No atomics, every sum in a fixed order: bit-reproducible, and a sequence's results do not depend on the rest of the batch.
//
// HEAD (recurrence launch only): where the step's upstream dH_t comes from.
//   SEB_HEAD_NONE  read from dH [B][Tn][F][N]
//   SEB_HEAD_LAST  the read-out on h_T: dH_T[i] = sum_c dlogits[b][c] head_w[c][i] (c ascending) seeds the carried dh before the time loop;
//                  every step's own upstream is the constant 0
//   SEB_HEAD_NODE  the per-node head on every state: dH_t[f][n] = sum_o node_w[o][f] dY[b][t][o][n] (o ascending), formed where dH is read
// Everything behind the upstream is the same code: with an exactly representable dH the three give the same bits.
#include "gcrnn_common.h"

namespace {

template <typename T> __device__ __forceinline__ T seb_exp(T v);
template <> __device__ __forceinline__ float seb_exp<float>(float v) { return expf(v); }
template <> __device__ __forceinline__ double seb_exp<double>(double v) { return exp(v); }

constexpr int SEB_THREADS = 1024;
constexpr int SEB_PASSES = 4;            // (F + 2) * N <= SEB_PASSES * SEB_THREADS and (F + 2) * (K * C + 1) <= SEB_PASSES * SEB_THREADS (host)
constexpr int SEB_ROW_LANES = 8;         // lanes that share one support row / column in the list sums
constexpr int SEB_WAVES = SEB_THREADS / 64;
constexpr int SEB_HEAD_NONE = 0, SEB_HEAD_LAST = 1, SEB_HEAD_NODE = 2;

// sum over the SEB_ROW_LANES lanes of a group, the same value in every lane, in a fixed order
template <typename T> __device__ __forceinline__ T seb_group_sum(T v) {
#pragma unroll
  for (int o = SEB_ROW_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, SEB_ROW_LANES);
  return v;
}

}  // namespace

template <typename T, bool XP, bool DX = false, int HEAD = SEB_HEAD_NONE>
__global__ __launch_bounds__(1024) void small_edge_bptt_kernel(
    const T* __restrict__ U,          // XP: X [B][Tn][C][N]        else: h0 [B][C][N]  (C = F)
    const T* __restrict__ Hs,         // [B][Tn][F][N] states of the forward (not XP)
    const T* __restrict__ dH,         // [B][Tn][F][N] upstream gradient (not XP); HEAD_LAST: dlogits [B][NC]; HEAD_NODE: dY [B][Tn][NC][N]
    const T* __restrict__ head_w,     // HEAD_LAST: [NC][F N]       HEAD_NODE: [NC][F]
    const T* __restrict__ w,          // [F][K][C] filter taps
    const T* __restrict__ bias,       // [F] or null
    const T* __restrict__ attW,       // [F][F]
    const T* __restrict__ attA,       // [2 F]  a1 | a2
    const T* __restrict__ gate,       // [Tn][B] or null            XP: gi, else: gf
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const T* __restrict__ val,          // CSR(S^T)
    const int32_t* __restrict__ a_rowptr, const int32_t* __restrict__ a_col, const T* __restrict__ a_val,    // CSR(S) (not XP, or DX)
    const int32_t* __restrict__ s_rowptr, const int2* __restrict__ r_edge,
    const int32_t* __restrict__ t_rowptr, const int2* __restrict__ t_edge, const T* __restrict__ t_val, const int32_t* __restrict__ t_pos,
    T* __restrict__ dPre,             // [B][Tn][F][N]              XP: read, else: written
    T* __restrict__ pwf,              // [gridDim.x][R][K][C] gradient of the folded taps
    T* __restrict__ pbf,              // [gridDim.x][R]       ... and of the folded bias
    T* __restrict__ dgate,            // [Tn][B] or null (with gate)
    T* __restrict__ dU,               // XP with DX: dX [B][Tn][C][N]   not XP: dh0 [B][F][N] or null
    int Tn, int N, int C, int F, int K, int nnz, int nnzs, int B, int NC) {
  static_assert(XP || !DX, "the gradient for X leaves the input branch");
  static_assert(!XP || HEAD == SEB_HEAD_NONE, "the heads sit on the state: recurrence launch only");
  constexpr bool HOPS = !XP || DX;                           // the hops' adjoint runs: CSR(S) in LDS
  extern __shared__ __attribute__((aligned(16))) char smem_small_edge_bwd[];
  const int R = F + 2;
  const int KC = K * C, CN = C * N, FN = F * N, RN = R * N;
  const int GN = (C > F ? C : F) * N;
  T* z = reinterpret_cast<T*>(smem_small_edge_bwd);          // [K][C][N]
  T* wf = z + (size_t)K * CN;                                // [R][K][C]
  T* bf = wf + (size_t)R * KC;                               // [R]
  T* wx = bf + R;                                            // [R][N]: Wx rows, then s1, then s2
  T* dwx = wx + RN;                                          // [R][N]: dWx rows, then ds1, then ds2
  T* mx = dwx + RN;                                          // [N]
  T* den = mx + N;                                           // [N]
  T* rsum = den + N;                                         // [N]
  T* coef = rsum + N;                                        // [nnzs]
  T* tvl = coef + nnzs;                                      // [nnzs]
  T* pz = tvl + nnzs;                                        // [nnzs] alpha dalpha, then dzz
  T* vall = pz + nnzs;                                       // [nnz]
  T* avl = vall + nnz;                                       // [nnz]
  T* gbuf0 = avl + nnz;                                      // [max(C, F)][N] dy / Horner ping
  T* gbuf1 = gbuf0 + GN;                                     // [max(C, F)][N] Horner pong
  T* red = gbuf1 + GN;                                       // [SEB_WAVES]
  int32_t* rpl = reinterpret_cast<int32_t*>(red + SEB_WAVES);   // [N + 1]
  int32_t* rrp = rpl + (N + 1);                              // [N + 1]
  int32_t* trp = rrp + (N + 1);                              // [N + 1]
  int32_t* arp = trp + (N + 1);                              // [N + 1]
  int32_t* coll = arp + (N + 1);                             // [nnz]
  int32_t* acl = coll + nnz;                                 // [nnz]
  int32_t* rcol = acl + nnz;                                 // [nnzs] column n of row-list entry j
  int32_t* tm = rcol + nnzs;                                 // [nnzs] row m of transposed-list edge q
  int32_t* tn = tm + nnzs;                                   // [nnzs] column n of transposed-list edge q
  int32_t* inv = tn + nnzs;                                  // [nnzs] transposed-list edge q of row-list entry j
  const int tid = threadIdx.x;
  const int b = XP ? (int)(blockIdx.x / (unsigned)Tn) : (int)blockIdx.x;
  const int t_only = XP ? (int)(blockIdx.x - (unsigned)b * (unsigned)Tn) : 0;
  const T* s1 = wx + (size_t)F * N;
  const T* s2 = s1 + N;

  for (int i = tid; i < nnz; i += SEB_THREADS) {
    vall[i] = val[i]; coll[i] = col[i];
    if (HOPS) { avl[i] = a_val[i]; acl[i] = a_col[i]; }
  }
  for (int i = tid; i < nnzs; i += SEB_THREADS) {
    tvl[i] = t_val[i]; rcol[i] = r_edge[i].x; tm[i] = t_edge[i].x;
    inv[t_pos[i]] = i;                                       // t_pos is a permutation: every entry written once
  }
  for (int i = tid; i <= N; i += SEB_THREADS) {
    rpl[i] = rowptr[i]; rrp[i] = s_rowptr[i]; trp[i] = t_rowptr[i];
    if (HOPS) arp[i] = a_rowptr[i];
  }
  // fold the attention's mixing matrix and mixer into the taps, as the forward does
  for (int i = tid; i < F * KC; i += SEB_THREADS) {
    const int f = i / KC, r = i - f * KC;
    T acc = T(0);
    for (int f2 = 0; f2 < F; ++f2) acc += attW[f * F + f2] * w[(size_t)f2 * KC + r];
    wf[i] = acc;
  }
  for (int f = tid; f < F; f += SEB_THREADS) {
    T acc = T(0);
    if (bias)
      for (int f2 = 0; f2 < F; ++f2) acc += attW[f * F + f2] * bias[f2];
    bf[f] = acc;
  }
  if (HEAD == SEB_HEAD_LAST) {                                                                   // dh after the last step: the read-out's dH_T (C = F: GN = FN)
    const T* dl = dH + (size_t)b * NC;
    for (int i = tid; i < GN; i += SEB_THREADS) {
      T acc = T(0);
      for (int c = 0; c < NC; ++c) acc += dl[c] * head_w[(size_t)c * FN + i];
      gbuf0[i] = acc;
    }
  } else {
    for (int i = tid; i < GN; i += SEB_THREADS) gbuf0[i] = T(0);                                 // dh after the last step
  }
  __syncthreads();
  for (int i = tid; i < 2 * KC; i += SEB_THREADS) {
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
  for (int n = tid; n < N; n += SEB_THREADS)
    for (int q = trp[n]; q < trp[n + 1]; ++q) tn[q] = n;
  // (the first barrier of the step loop orders these writes before their readers)

  int of[SEB_PASSES], on[SEB_PASSES];                        // outputs of the tap pass (R N) and, the first F N, of the column pass
  T dwacc[SEB_PASSES];                                       // outputs of the tap adjoint: i = r (KC + 1) + kc, kc == KC for the bias
  const int NW = R * (KC + 1);
#pragma unroll
  for (int p = 0; p < SEB_PASSES; ++p) {
    const int i = tid + p * SEB_THREADS;
    of[p] = i / N;
    on[p] = i - of[p] * N;
    dwacc[p] = T(0);
  }
  const int grp = tid / SEB_ROW_LANES, grp_lane = tid & (SEB_ROW_LANES - 1);
  T* cur = gbuf0;                                            // dh, then dy of the step
  T* oth = gbuf1;

  const int t_hi = XP ? t_only : Tn - 1, t_lo = XP ? t_only : 0;
  for (int t = t_hi; t >= t_lo; --t) {
    {
      const T* u0 = XP ? U + ((size_t)b * Tn + t) * CN : (t > 0 ? Hs + ((size_t)b * Tn + (t - 1)) * FN : U + (size_t)b * FN);
      for (int i = tid; i < CN; i += SEB_THREADS) z[i] = u0[i];                                 // z_0 = x_t or h_{t-1}
    }
    if (HEAD == SEB_HEAD_NODE) {
      // the step's upstream dH_t[f][n] = sum_o node_w[o][f] dY[b][t][o][n], o ascending, parked in dwx (free until the column pass's adjoint):
      // element i is written and read back by the same thread, here where few registers are live
      const T* dyt = dH + ((size_t)b * Tn + t) * NC * N;
      for (int i = tid; i < FN; i += SEB_THREADS) {
        const int f = i / N, n = i - f * N;
        T s = T(0);
        for (int c = 0; c < NC; ++c) s += head_w[c * F + f] * dyt[c * N + n];
        dwx[i] = s;
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- the step's forward, as small_edge_cell_kernel
    for (int k = 1; k < K; ++k) {
      const T* zp = z + (size_t)(k - 1) * CN;
      T* zn = z + (size_t)k * CN;
      for (int i = tid; i < CN; i += SEB_THREADS) {
        const int c = i / N, n = i - c * N;
        const T* zr = zp + c * N;
        T acc = T(0);
        for (int j = rpl[n]; j < rpl[n + 1]; ++j) acc += vall[j] * zr[coll[j]];
        zn[i] = acc;
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < SEB_PASSES; ++p) {
      const int i = tid + p * SEB_THREADS;
      if (i < RN) {
        const T* wr = wf + of[p] * KC;
        const T* zc = z + on[p];
        T acc = bf[of[p]];
        for (int kc = 0; kc < KC; ++kc) acc += wr[kc] * zc[kc * N];
        wx[i] = acc;
      }
    }
    __syncthreads();
    for (int m = grp; m < N; m += SEB_THREADS / SEB_ROW_LANES) {
      const int j0 = rrp[m], j1 = rrp[m + 1];
      const T z2 = s2[m];
      T mv = (T)(-INFINITY);
      for (int j = j0 + grp_lane; j < j1; j += SEB_ROW_LANES) {
        const T zz = s1[rcol[j]] + z2;
        const T e = zz > T(0) ? zz : T(0.2) * zz;
        mv = e > mv ? e : mv;
      }
#pragma unroll
      for (int o = SEB_ROW_LANES / 2; o > 0; o >>= 1) {
        const T other = __shfl_xor(mv, o, SEB_ROW_LANES);
        mv = other > mv ? other : mv;
      }
      T d = T(0);
      for (int j = j0 + grp_lane; j < j1; j += SEB_ROW_LANES) {
        const T zz = s1[rcol[j]] + z2;
        const T e = zz > T(0) ? zz : T(0.2) * zz;
        d += seb_exp<T>(e - mv);
      }
      d = seb_group_sum<T>(d);
      if (grp_lane == 0) { mx[m] = mv; den[m] = d; }
    }
    __syncthreads();
    for (int q = tid; q < nnzs; q += SEB_THREADS) {
      const int m = tm[q];
      const T zz = s1[tn[q]] + s2[m];
      const T e = zz > T(0) ? zz : T(0.2) * zz;
      coef[q] = tvl[q] * (seb_exp<T>(e - mx[m]) / den[m]);
    }
    __syncthreads();
    // ---------------------------------------------------------------- column pass again, the step's upstream, dy
    T g = T(1);
    if (gate) g = gate[(size_t)t * B + b];
    T part = T(0);
    T hv[SEB_PASSES], up[SEB_PASSES];                         // h_t and the upstream gradient: in flight during the column sums
    {
      const size_t o = ((size_t)b * Tn + t) * FN;
#pragma unroll
      for (int p = 0; p < SEB_PASSES; ++p) {
        const int i = tid + p * SEB_THREADS;
        hv[p] = (!XP && i < FN) ? Hs[o + i] : T(0);
        if (HEAD == SEB_HEAD_NONE) {
          up[p] = (i < FN) ? (XP ? dPre[o + i] : dH[o + i]) : T(0);
        } else {
          up[p] = T(0);                                       // HEAD_LAST: the constant; HEAD_NODE: formed behind the column sum below
        }
      }
    }
#pragma unroll
    for (int p = 0; p < SEB_PASSES; ++p) {
      const int i = tid + p * SEB_THREADS;
      if (i < FN) {
        const int n = on[p];
        const T* wr = wx + of[p] * N;
        T acc = T(0);
        for (int q = trp[n]; q < trp[n + 1]; ++q) acc += coef[q] * wr[tm[q]];
        T dpre;
        if (XP) {
          dpre = up[p];
        } else {
          if (HEAD == SEB_HEAD_NODE) up[p] = dwx[i];          // formed on top of the step, this thread's own element
          dpre = (up[p] + cur[i]) * (T(1) - hv[p] * hv[p]);
          dPre[((size_t)b * Tn + t) * FN + i] = dpre;
        }
        const bool on_ = acc > T(0);
        part += on_ ? dpre * acc : T(0);
        cur[i] = on_ ? g * dpre : T(0);                       // dy (C = F without XP: element i is this thread's own)
      }
    }
    if (gate) {                                               // (uniform) d loss / d gate: wave butterflies, then the waves in order
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      if ((tid & 63) == 0) red[tid >> 6] = part;
    }
    __syncthreads();
    if (gate && tid == 0) {
      T s = T(0);
      for (int i = 0; i < SEB_WAVES; ++i) s += red[i];
      dgate[(size_t)t * B + b] = s;
    }
    // ---------------------------------------------------------------- adjoint of the column pass
    for (int q = tid; q < nnzs; q += SEB_THREADS) {
      const T* dyc = cur + tn[q];
      const T* wc = wx + tm[q];
      T acc = T(0);
      for (int f = 0; f < F; ++f) acc += dyc[f * N] * wc[f * N];
      pz[q] = coef[q] * acc;                                  // alpha dalpha = coef dcoef
    }
#pragma unroll
    for (int p = 0; p < SEB_PASSES; ++p) {
      const int i = tid + p * SEB_THREADS;
      if (i < FN) {
        const int m = on[p];
        const T* dyr = cur + of[p] * N;
        T acc = T(0);
        for (int j = rrp[m]; j < rrp[m + 1]; ++j) acc += coef[inv[j]] * dyr[rcol[j]];
        dwx[i] = acc;
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- adjoint of the masked softmax and the LeakyReLU
    for (int m = grp; m < N; m += SEB_THREADS / SEB_ROW_LANES) {
      T s = T(0);
      for (int j = rrp[m] + grp_lane; j < rrp[m + 1]; j += SEB_ROW_LANES) s += pz[inv[j]];
      s = seb_group_sum<T>(s);
      if (grp_lane == 0) rsum[m] = s;
    }
    __syncthreads();
    for (int q = tid; q < nnzs; q += SEB_THREADS) {
      const int m = tm[q];
      const T zz = s1[tn[q]] + s2[m];
      const T e = zz > T(0) ? zz : T(0.2) * zz;
      const T alpha = seb_exp<T>(e - mx[m]) / den[m];
      const T de = pz[q] - alpha * rsum[m];
      pz[q] = zz > T(0) ? de : T(0.2) * de;
    }
    __syncthreads();
    for (int it = grp; it < 2 * N; it += SEB_THREADS / SEB_ROW_LANES) {
      T s = T(0);
      if (it < N) {                                           // ds1[n]: column n of the support
        for (int q = trp[it] + grp_lane; q < trp[it + 1]; q += SEB_ROW_LANES) s += pz[q];
      } else {                                                // ds2[m]: row m
        const int m = it - N;
        for (int j = rrp[m] + grp_lane; j < rrp[m + 1]; j += SEB_ROW_LANES) s += pz[inv[j]];
      }
      s = seb_group_sum<T>(s);
      if (grp_lane == 0) dwx[FN + it] = s;
    }
    __syncthreads();
    // ---------------------------------------------------------------- adjoint of the folded tap pass (weights: registers, all steps)
#pragma unroll
    for (int p = 0; p < SEB_PASSES; ++p) {
      const int i = tid + p * SEB_THREADS;
      if (i < NW) {
        const int r = i / (KC + 1), kc = i - r * (KC + 1);
        const T* dr = dwx + r * N;
        T acc = T(0);
        int n = i % N;                                        // lanes start their sums at different nodes: the LDS reads spread over the banks
        if (kc < KC) {
          const T* zr = z + (size_t)kc * N;
          for (int c = 0; c < N; ++c) {
            acc += dr[n] * zr[n];
            n = n + 1 == N ? 0 : n + 1;
          }
        } else {
          for (int c = 0; c < N; ++c) {
            acc += dr[n];
            n = n + 1 == N ? 0 : n + 1;
          }
        }
        dwacc[p] += acc;
      }
    }
    if (HOPS) {
      // -------------------------------------------------------------- adjoint of the hops, Horner form; g_0 is the new dh (DX: dX_t)
      const T* src = nullptr;
      for (int k = K - 1; k >= 0; --k) {
        T* dst = oth;
        for (int i = tid; i < CN; i += SEB_THREADS) {
          const int c = i / N, n = i - c * N;
          const T* wc = wf + k * C + c;
          const T* dc = dwx + n;
          T acc = T(0);
          for (int r = 0; r < R; ++r) acc += wc[r * KC] * dc[r * N];
          if (src) {
            const T* gr = src + c * N;
            for (int j = arp[n]; j < arp[n + 1]; ++j) acc += avl[j] * gr[acl[j]];
          }
          dst[i] = acc;
        }
        __syncthreads();
        src = dst;
        oth = cur;
        cur = dst;
      }
      if (DX) {
        T* dx = dU + ((size_t)b * Tn + t) * CN;
        for (int i = tid; i < CN; i += SEB_THREADS) dx[i] = cur[i];
      }
    } else {
      __syncthreads();
    }
  }
#pragma unroll
  for (int p = 0; p < SEB_PASSES; ++p) {
    const int i = tid + p * SEB_THREADS;
    if (i < NW) {
      const int r = i / (KC + 1), kc = i - r * (KC + 1);
      if (kc < KC) pwf[(size_t)blockIdx.x * R * KC + (size_t)r * KC + kc] = dwacc[p];
      else pbf[(size_t)blockIdx.x * R + r] = dwacc[p];
    }
  }
  if (!XP && dU)
    for (int i = tid; i < FN; i += SEB_THREADS) dU[(size_t)b * FN + i] = cur[i];
}

static size_t small_edge_bwd_lds_bytes(int dtype, int64_t N, int64_t nnz, int64_t nnzs, int64_t G, int64_t F, int64_t Kin, int64_t Kst) {
  const size_t e = dtype == GCRNN_F64 ? 8 : 4;
  const int64_t K = Kin > Kst ? Kin : Kst, C = G > F ? G : F, R = F + 2;
  return e * (size_t)(K * C * N + R * K * C + R + 2 * R * N + 3 * N + 3 * nnzs + 2 * nnz + 2 * C * N + SEB_WAVES) +
         4 * (size_t)(4 * (N + 1) + 2 * nnz + 4 * nnzs) + 16;
}

extern "C" int gcrnn_small_edge_backward_supported(int dtype, int64_t N, int64_t nnz, int64_t nnz_support, int64_t G, int64_t F,
                                                   int64_t Kin, int64_t Kst) {
  if (!gcrnn_small_edge_supported(dtype, N, nnz, nnz_support, G, F, Kin, Kst)) return 0;
  const int64_t K = Kin > Kst ? Kin : Kst, C = G > F ? G : F;
  // this file's own limits, whatever the forward's constants are: the R N outputs of the tap pass and of the column pass's adjoint
  // take SEB_PASSES passes of the workgroup, and the regime is that of the forward (N <= 128)
  if (N > 128 || (F + 2) * N > SEB_PASSES * SEB_THREADS) return 0;
  // the folded taps' gradient (and the folded bias') lives in SEB_PASSES registers per thread
  if ((F + 2) * (K * C + 1) > SEB_PASSES * SEB_THREADS) return 0;
  return small_edge_bwd_lds_bytes(dtype, N, nnz, nnz_support, G, F, Kin, Kst) <= 150 * 1024 ? 1 : 0;
}

namespace {
struct SmallEdgeBwdArgs {
  const void *X, *h0, *H, *dH, *head_w, *wA, *wB, *bias, *att_in_w, *att_in_a, *att_f_w, *att_f_a, *gi, *gf;
  const int32_t *rowptr, *col;
  const void* val;
  const int32_t *a_rowptr, *a_col;
  const void* a_val;
  const int32_t *s_rowptr, *r_edge, *t_rowptr, *t_edge;
  const void* t_val;
  const int32_t* t_pos;
  void *dPre, *pwfA, *pbfA, *pwfB, *pbfB, *dgi, *dgf, *dh0, *dX;
  int64_t B, T, N, G, F, Kin, Kst, nnz, nnzs, NC;
};
}  // namespace

template <typename T, bool DX, int HEAD>
static int small_edge_bwd_launch(const SmallEdgeBwdArgs& a, size_t lds, hipStream_t st) {
  auto kx = small_edge_bptt_kernel<T, true, DX>;
  auto kh = small_edge_bptt_kernel<T, false, false, HEAD>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(kh), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GCRNN_ERR_LAUNCH;
  GCRNN_PRE_LAUNCH();
  kh<<<(unsigned)a.B, SEB_THREADS, lds, st>>>((const T*)a.h0, (const T*)a.H, (const T*)a.dH, (const T*)a.head_w, (const T*)a.wB,
                                              (const T*)a.bias, (const T*)a.att_f_w, (const T*)a.att_f_a, (const T*)a.gf, a.rowptr, a.col,
                                              (const T*)a.val, a.a_rowptr, a.a_col, (const T*)a.a_val, a.s_rowptr, (const int2*)a.r_edge,
                                              a.t_rowptr, (const int2*)a.t_edge, (const T*)a.t_val, a.t_pos, (T*)a.dPre, (T*)a.pwfB,
                                              (T*)a.pbfB, (T*)a.dgf, (T*)a.dh0, (int)a.T, (int)a.N, (int)a.F, (int)a.F, (int)a.Kst,
                                              (int)a.nnz, (int)a.nnzs, (int)a.B, (int)a.NC);
  // the input branch reads CSR(S) only for dX
  kx<<<(unsigned)(a.B * a.T), SEB_THREADS, lds, st>>>((const T*)a.X, (const T*)nullptr, (const T*)nullptr, (const T*)nullptr,
                                                      (const T*)a.wA, (const T*)a.bias, (const T*)a.att_in_w, (const T*)a.att_in_a,
                                                      (const T*)a.gi, a.rowptr, a.col, (const T*)a.val, DX ? a.a_rowptr : nullptr,
                                                      DX ? a.a_col : nullptr, DX ? (const T*)a.a_val : nullptr, a.s_rowptr,
                                                      (const int2*)a.r_edge, a.t_rowptr, (const int2*)a.t_edge, (const T*)a.t_val, a.t_pos,
                                                      (T*)a.dPre, (T*)a.pwfA, (T*)a.pbfA, (T*)a.dgi, DX ? (T*)a.dX : (T*)nullptr,
                                                      (int)a.T, (int)a.N, (int)a.G, (int)a.F, (int)a.Kin, (int)a.nnz, (int)a.nnzs,
                                                      (int)a.B, 0);
  GCRNN_CHECK_LAUNCH();
  return GCRNN_OK;
}

template <typename T, bool DX>
static int small_edge_bwd_launch_head(const SmallEdgeBwdArgs& a, int head_kind, size_t lds, hipStream_t st) {
  if (head_kind == SEB_HEAD_LAST) return small_edge_bwd_launch<T, DX, SEB_HEAD_LAST>(a, lds, st);
  if (head_kind == SEB_HEAD_NODE) return small_edge_bwd_launch<T, DX, SEB_HEAD_NODE>(a, lds, st);
  return small_edge_bwd_launch<T, DX, SEB_HEAD_NONE>(a, lds, st);
}

// all entry points: the validation, then the two launches. need_dx: dX is one more required pointer (gcrnn_small_edge_backward_dx);
// head: gcrnn_small_edge_backward_head, a.dH is the head's upstream and a.dX selects the input branch's dx variant
static int small_edge_backward(int dtype, const SmallEdgeBwdArgs& a, bool need_dx, bool head, int head_kind, void* stream) {
  if (!a.X || !a.h0 || !a.H || !a.dH || !a.wA || !a.wB || !a.att_in_w || !a.att_in_a || !a.att_f_w || !a.att_f_a || !a.rowptr ||
      !a.a_rowptr || !a.s_rowptr || !a.t_rowptr || !a.dPre || !a.pwfA || !a.pbfA || !a.pwfB || !a.pbfB || (need_dx && !a.dX) ||
      (head && !a.head_w))
    return GCRNN_ERR_NULL_POINTER;
  if ((a.nnz > 0 && (!a.col || !a.val || !a.a_col || !a.a_val)) || (a.nnzs > 0 && (!a.r_edge || !a.t_edge || !a.t_val || !a.t_pos)))
    return GCRNN_ERR_NULL_POINTER;
  if ((a.gi == nullptr) != (a.gf == nullptr)) return GCRNN_ERR_NULL_POINTER;
  if (a.gi && (!a.dgi || !a.dgf)) return GCRNN_ERR_NULL_POINTER;
  if (dtype != GCRNN_F32 && dtype != GCRNN_F64) return GCRNN_ERR_BAD_DTYPE;
  if (a.B <= 0 || a.T <= 0 || a.N <= 0 || a.G <= 0 || a.F <= 0 || a.Kin <= 0 || a.Kst <= 0 || a.nnz < 0 || a.nnzs < 0)
    return GCRNN_ERR_BAD_SHAPE;
  if (a.B > 2147483647LL || a.T > 2147483647LL || a.B * a.T > 2147483647LL) return GCRNN_ERR_BAD_SHAPE;
  if (head) {
    if (head_kind != SEB_HEAD_LAST && head_kind != SEB_HEAD_NODE) return GCRNN_ERR_BAD_SHAPE;
    if (a.NC <= 0 || a.NC > (head_kind == SEB_HEAD_NODE ? GCRNN_SMALL_NODE_HEAD_MAX_OUT : GCRNN_SMALL_HEAD_MAX_CLASSES))
      return GCRNN_ERR_BAD_SHAPE;
    if (!gcrnn_small_edge_head_supported(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst, head_kind, a.NC, 1))
      return GCRNN_ERR_UNSUPPORTED;
  } else if (!gcrnn_small_edge_backward_supported(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst)) {
    return GCRNN_ERR_UNSUPPORTED;
  }
  const size_t lds = small_edge_bwd_lds_bytes(dtype, a.N, a.nnz, a.nnzs, a.G, a.F, a.Kin, a.Kst);
  hipStream_t st = as_stream(stream);
  const bool dx = a.dX != nullptr;
  if (dtype == GCRNN_F32)
    return dx ? small_edge_bwd_launch_head<float, true>(a, head_kind, lds, st) : small_edge_bwd_launch_head<float, false>(a, head_kind, lds, st);
  return dx ? small_edge_bwd_launch_head<double, true>(a, head_kind, lds, st) : small_edge_bwd_launch_head<double, false>(a, head_kind, lds, st);
}

extern "C" int gcrnn_small_edge_backward(int dtype, const void* X, const void* h0, const void* H, const void* dH, const void* wA,
                                         const void* wB, const void* bias, const void* att_in_w, const void* att_in_a,
                                         const void* att_f_w, const void* att_f_a, const void* gi, const void* gf,
                                         const int32_t* rowptr, const int32_t* col, const void* val, const int32_t* a_rowptr,
                                         const int32_t* a_col, const void* a_val, const int32_t* s_rowptr, const int32_t* r_edge,
                                         const int32_t* t_rowptr, const int32_t* t_edge, const void* t_val, const int32_t* t_pos,
                                         void* dPre, void* pwfA, void* pbfA, void* pwfB, void* pbfB, void* dgi, void* dgf, void* dh0,
                                         int64_t B, int64_t T, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst, int64_t nnz,
                                         int64_t nnz_support, void* stream) {
  const SmallEdgeBwdArgs a = {X, h0, H, dH, nullptr, wA, wB, bias, att_in_w, att_in_a, att_f_w, att_f_a, gi, gf, rowptr, col, val, a_rowptr,
                              a_col, a_val, s_rowptr, r_edge, t_rowptr, t_edge, t_val, t_pos, dPre, pwfA, pbfA, pwfB, pbfB, dgi, dgf, dh0,
                              nullptr, B, T, N, G, F, Kin, Kst, nnz, nnz_support, 0};
  return small_edge_backward(dtype, a, false, false, SEB_HEAD_NONE, stream);
}

extern "C" int gcrnn_small_edge_backward_dx(int dtype, const void* X, const void* h0, const void* H, const void* dH, const void* wA,
                                            const void* wB, const void* bias, const void* att_in_w, const void* att_in_a,
                                            const void* att_f_w, const void* att_f_a, const void* gi, const void* gf,
                                            const int32_t* rowptr, const int32_t* col, const void* val, const int32_t* a_rowptr,
                                            const int32_t* a_col, const void* a_val, const int32_t* s_rowptr, const int32_t* r_edge,
                                            const int32_t* t_rowptr, const int32_t* t_edge, const void* t_val, const int32_t* t_pos,
                                            void* dPre, void* pwfA, void* pbfA, void* pwfB, void* pbfB, void* dgi, void* dgf, void* dh0,
                                            void* dX, int64_t B, int64_t T, int64_t N, int64_t G, int64_t F, int64_t Kin, int64_t Kst,
                                            int64_t nnz, int64_t nnz_support, void* stream) {
  const SmallEdgeBwdArgs a = {X, h0, H, dH, nullptr, wA, wB, bias, att_in_w, att_in_a, att_f_w, att_f_a, gi, gf, rowptr, col, val, a_rowptr,
                              a_col, a_val, s_rowptr, r_edge, t_rowptr, t_edge, t_val, t_pos, dPre, pwfA, pbfA, pwfB, pbfB, dgi, dgf, dh0,
                              dX, B, T, N, G, F, Kin, Kst, nnz, nnz_support, 0};
  return small_edge_backward(dtype, a, true, false, SEB_HEAD_NONE, stream);
}

extern "C" int gcrnn_small_edge_backward_head(int dtype, const void* X, const void* h0, const void* H, const void* up, const void* head_w,
                                              const void* wA, const void* wB, const void* bias, const void* att_in_w,
                                              const void* att_in_a, const void* att_f_w, const void* att_f_a, const void* gi,
                                              const void* gf, const int32_t* rowptr, const int32_t* col, const void* val,
                                              const int32_t* a_rowptr, const int32_t* a_col, const void* a_val, const int32_t* s_rowptr,
                                              const int32_t* r_edge, const int32_t* t_rowptr, const int32_t* t_edge, const void* t_val,
                                              const int32_t* t_pos, void* dPre, void* pwfA, void* pbfA, void* pwfB, void* pbfB, void* dgi,
                                              void* dgf, void* dh0, void* dX, int64_t B, int64_t T, int64_t N, int64_t G, int64_t F,
                                              int64_t Kin, int64_t Kst, int64_t nnz, int64_t nnz_support, int64_t NC, int head_kind,
                                              void* stream) {
  const SmallEdgeBwdArgs a = {X, h0, H, up, head_w, wA, wB, bias, att_in_w, att_in_a, att_f_w, att_f_a, gi, gf, rowptr, col, val, a_rowptr,
                              a_col, a_val, s_rowptr, r_edge, t_rowptr, t_edge, t_val, t_pos, dPre, pwfA, pbfA, pwfB, pbfB, dgi, dgf, dh0,
                              dX, B, T, N, G, F, Kin, Kst, nnz, nnz_support, NC};
  return small_edge_backward(dtype, a, false, true, head_kind, stream);
}
