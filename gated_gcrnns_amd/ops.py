"""torch.autograd bindings over the C ABI (include/gcrnn.h).

Everything here moves raw device pointers into libgcrnn_hip.so on the current
HIP stream; torch only owns the memory. CPU tensors are rejected: the product
has no CPU path (the CPU restatement lives in oracle/ and is test-only).

Node-major layout used by every op: X[T][N][B][C] (see include/gcrnn.h).
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import lib, check, dtype_code, GcrnnError


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GcrnnError('gated_gcrnns_amd has no CPU path: move the module and its inputs to a ROCm '
                             'device (model.to("cuda"), x.cuda()); got a tensor on %s' % t.device)


# ------------------------------------------------------------------------------------------ layout
def _pack_raw(x, perm=None):
    B, T, Cc, N = x.shape
    out = torch.empty((T, N, B, Cc), dtype=x.dtype, device=x.device)
    check(lib.gcrnn_pack_node_major(dtype_code(x.dtype), _p(x), _p(out), B, T, Cc, N, _p(perm), _stream()), 'pack')
    return out


def _unpack_raw(X, perm=None):
    T, N, B, Cc = X.shape
    out = torch.empty((B, T, Cc, N), dtype=X.dtype, device=X.device)
    check(lib.gcrnn_unpack_node_major(dtype_code(X.dtype), _p(X), _p(out), B, T, Cc, N, _p(perm), _stream()), 'unpack')
    return out


class _Pack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _pack_raw(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return _unpack_raw(g.contiguous())


class _Unpack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X):
        return _unpack_raw(X.contiguous())

    @staticmethod
    def backward(ctx, g):
        return _pack_raw(g.contiguous())


def pack_node_major(x):
    """user [B][T][C][N] -> node-major [T][N][B][C]"""
    require_device(x)
    assert x.dim() == 4
    return _Pack.apply(x)


def unpack_node_major(X):
    """node-major [T][N][B][C] -> user [B][T][C][N]"""
    require_device(X)
    assert X.dim() == 4
    return _Unpack.apply(X)


# ------------------------------------------------------------------------------------------ shift
_SPMM_TUNE = {}      # {'piece_lanes': .., 'unroll': .., 'rows_per_wave': ..}: overrides for tuning sweeps (tools/spmm_sweep.py)


def spmm_auto_tune(csr, L, elt):
    """Piece width / loads in flight of the streaming SpMM from what the host knows (the kernel's own default knows neither the
    mean degree nor where the operand lives). Dense neighbourhoods on an operand far beyond L2 (cfg5: ~100 non-zeros per row,
    51 MB): 128-byte pieces, 8 slots x 8 loads (measured best, tools/spmm_sweep.py). Sparse rows (cfg2: ~10 per row) on wide
    node rows: whole-wave pieces and as many loads in flight as a row has neighbours, otherwise most slots idle."""
    deg = csr.nnz / max(csr.N, 1)
    row_bytes = L * elt
    lanes = max(4, min(64, 1 << max(0, (row_bytes // 16 - 1)).bit_length()))        # lanes that cover one row (power of two)
    if csr.N * row_bytes > (8 << 20) and deg >= 32:
        return dict(piece_lanes=min(lanes, 8), unroll=8, rows_per_wave=4)
    slots = 64 // lanes
    unroll = 8 if deg > 16 * slots else (4 if deg > 2 * slots else 2)                # measured at cfg2 (deg 10, 1 KiB pieces): 4 beats 8
    if unroll == 2 and lanes > 8:
        unroll = 4                                                                   # (2-deep variants are built for narrow pieces only)
    return dict(piece_lanes=lanes, unroll=unroll, rows_per_wave=1 if csr.N <= 4096 else 4)


def spmm_raw(csr, X, out=None, accumulate=False, bias=None, bias_scale=0.0, tanh=False, tune=None):
    """Y[i][n][:] (+)= sum_j val[j] X[i][col[j]][:] on a contiguous [nbatch][N][L...] tensor (bf16 / fp32 / fp64 rows; the
    CSR weights are fp32 for bf16 rows). tanh: Y = tanh(. + bias_scale * bias[l % F]) -- the last hop of a Horner-form step
    (bias: [F] in the weights' dtype or None). Rows that are whole 16-byte vectors run on the streaming kernel
    (gcrnn_spmm_ex); other shapes fall back to the scalar kernel (no epilogue there)."""
    N = csr.N
    assert X.is_contiguous() and X.dim() >= 3
    nbatch = X.shape[0]
    assert X.shape[1] == N, 'node-major tensor has %d rows, graph has %d nodes' % (X.shape[1], N)
    L = X[0, 0].numel()
    if out is None:
        assert not accumulate
        out = torch.empty_like(X)
    ve = 16 // X.element_size()
    if L % ve == 0 and X.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0:
        t = tune if tune is not None else (_SPMM_TUNE or spmm_auto_tune(csr, L, X.element_size()))
        F = bias.numel() if bias is not None else 0
        check(lib.gcrnn_spmm_ex(dtype_code(X.dtype), N, _p(csr.rowptr), _p(csr.col), _p(csr.val(X.dtype)), _p(X), _p(out),
                                L, nbatch, int(accumulate), _p(bias), float(bias_scale), F, int(tanh),
                                int(t.get('piece_lanes', 0)), int(t.get('unroll', 0)), int(t.get('rows_per_wave', 0)), _stream()), 'spmm_ex')
        return out
    check(lib.gcrnn_spmm(dtype_code(X.dtype), N, _p(csr.rowptr), _p(csr.col), _p(csr.val(X.dtype)), _p(X), _p(out),
                         L, nbatch, int(accumulate), _stream()), 'spmm')
    if tanh:
        if bias is not None:
            out.add_(bias_scale * bias.view(-1).repeat(L // bias.numel()).view(out.shape[2:]))
        torch.tanh(out, out=out)
    return out


def taps_bf16_supported(F, G, K):
    return bool(lib.gcrnn_taps_bf16_supported(int(F), int(G), int(K)))


def taps_bf16(zh, zx, wA, wB, out0=None):
    """All K = max(Kin, Kst) taps of a Horner-form step in one pass on the matrix cores: u_k = zh B_k^T + zx A_k^T.
    zh [..][F], zx [..][G] bf16 node-major rows (same leading shape; zx None for a state-only operand), wA F x 1 x Kin x G,
    wB F x 1 x Kst x F (bf16 or fp32). Returns (u_0 [..][F], u_rest [K-1][..][F]) bf16; out0: where tap 0 is written."""
    F = wB.shape[0]
    G = wA.shape[3] if zx is not None else 0
    K = max(wA.shape[2], wB.shape[2])
    st = _stream()
    if zx is not None:
        wpack = _fused_pack_weights(wA.detach(), wB.detach(), st)
    else:
        wpack = _fused_pack_state_taps(wB, K, st)
    zh = zh.contiguous()
    zx = zx.contiguous() if zx is not None else None
    R = zh.numel() // F
    if out0 is None:
        out0 = torch.empty_like(zh)
    rest = torch.empty((max(K - 1, 1),) + tuple(zh.shape), dtype=torch.bfloat16, device=zh.device)
    check(lib.gcrnn_taps_bf16_forward(_p(zh), _p(zx), _p(wpack), _p(out0), _p(rest), R, F, G, K, st), 'taps_bf16')
    return out0, rest


def taps_mfma_supported(dtype, F, Ch, Cx):
    return dtype in (torch.float32, torch.float64) and bool(lib.gcrnn_taps_mfma_supported(dtype_code(dtype), int(F), int(Ch), int(Cx)))


def taps_mfma(zh, zx, wA, wB, out0=None):
    """fp32 / fp64 counterpart of taps_bf16 on the fp32 / fp64 matrix cores (gcrnn_taps_mfma_forward): all
    K = max(Kin, Kst) taps u_k = zh B_k^T + zx A_k^T of a Horner-form step. zh [..][F], zx [..][G] node-major rows, wA
    F x 1 x Kin x G, wB F x 1 x Kst x F in the rows' dtype. Returns (u_0, u_rest [K-1][..][F])."""
    F, Ch = wB.shape[0], wB.shape[3]
    Cx = wA.shape[3] if zx is not None else 0
    Kst, Kin = wB.shape[2], (wA.shape[2] if zx is not None else 0)
    K = max(Kin, Kst)
    zh = zh.contiguous()
    zx = zx.contiguous() if zx is not None else None
    wBc = wB.detach().contiguous()
    wAc = wA.detach().contiguous() if zx is not None else None
    R = zh.numel() // Ch
    if out0 is None:
        out0 = torch.empty(tuple(zh.shape[:-1]) + (F,), dtype=zh.dtype, device=zh.device)
    rest = torch.empty((max(K - 1, 1),) + tuple(out0.shape), dtype=zh.dtype, device=zh.device)
    check(lib.gcrnn_taps_mfma_forward(dtype_code(zh.dtype), _p(zh), _p(zx), _p(wBc), _p(wAc), _p(out0), _p(rest), R, F, Ch, Cx,
                                      Kst, Kin, _stream()), 'taps_mfma')
    return out0, rest


def taps_rows(z, w, out=None, accumulate=False):
    """y[r][:] (+)= z[r][:] w^T on node-major rows with the LDS-tiled tap kernel (fp32 / fp64): z [..][C], w [F][C]."""
    Cin = z.shape[-1]
    F = w.shape[0]
    z, w = z.contiguous(), w.contiguous()
    rows = z.numel() // Cin
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(z.shape[:-1]) + (F,), dtype=z.dtype, device=z.device)
    check(lib.gcrnn_taps_forward(dtype_code(z.dtype), _p(z), None, 0, _p(w), None, 0.0, _p(out), rows, 1, Cin, F,
                                 int(accumulate), _stream()), 'taps_forward')
    return out


class _Shift(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, fwd, adj):
        ctx.adj = adj
        return spmm_raw(fwd, X.contiguous())

    @staticmethod
    def backward(ctx, g):
        return spmm_raw(ctx.adj, g.contiguous()), None, None


def graph_shift(X, graph, e=0):
    """One application of the GSO on node-major data: the reference's x @ S_e (graphML.py:123)."""
    require_device(X)
    return _Shift.apply(X, graph.fwd[e], graph.adj[e])


# ------------------------------------------------------------------------------------------ LSIGF
class _LSIGF(torch.autograd.Function):
    """Node-major linear shift-invariant graph filter (graphML.py:47-140) for all E, K.

    forward : hops z_{e,k} = P_e z_{e,k-1} (CSR(S_e^T) SpMM), then one tap GEMM per edge feature.
    backward: dz = dy W (tap GEMM), reverse hop chain with CSR(S_e) in Horner form, dW by a
              row-reduction GEMM. The hop matrices are saved, not recomputed.
    """

    @staticmethod
    def forward(ctx, X, w, bias, graph, bias_scale):
        T, N, B, G = X.shape
        F, E, K, Gw = w.shape
        assert Gw == G and E == graph.E and N == graph.N
        dt = dtype_code(X.dtype)
        X = X.contiguous()
        rows = T * N * B
        zstride = rows * G
        zrest = torch.empty((E, max(K - 1, 1), T, N, B, G), dtype=X.dtype, device=X.device) if K > 1 else None
        y = torch.empty((T, N, B, F), dtype=X.dtype, device=X.device)
        wc = w.contiguous()
        bvec = bias.contiguous().view(-1) if bias is not None else None
        st = _stream()
        for e in range(E):
            src = X
            for k in range(1, K):
                spmm_raw(graph.fwd[e], src, out=zrest[e, k - 1])
                src = zrest[e, k - 1]
            we = wc[:, e].contiguous() if E > 1 else wc
            check(lib.gcrnn_taps_forward(dt, _p(X), _p(zrest[e]) if K > 1 else None, zstride, _p(we),
                                         _p(bvec) if e == 0 else None, float(bias_scale), _p(y), rows, K, G, F,
                                         int(e > 0), st), 'taps_forward')
        ctx.save_for_backward(X, zrest, wc)
        ctx.graph = graph
        ctx.has_bias = bias is not None
        ctx.bias_shape = tuple(bias.shape) if bias is not None else None
        ctx.bias_scale = float(bias_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        X, zrest, wc = ctx.saved_tensors
        graph = ctx.graph
        T, N, B, G = X.shape
        F, E, K, _ = wc.shape
        dt = dtype_code(X.dtype)
        dy = dy.contiguous()
        rows = T * N * B
        zstride = rows * G
        st = _stream()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        dX = None
        dW = torch.zeros_like(wc) if (need_w and E > 1) else None
        db = None
        for e in range(E):
            we = wc[:, e].contiguous() if E > 1 else wc
            if need_x:
                dz0 = torch.empty_like(X)
                dzr = torch.empty((max(K - 1, 1), T, N, B, G), dtype=X.dtype, device=X.device) if K > 1 else None
                check(lib.gcrnn_taps_backward_data(dt, _p(dy), _p(we), _p(dz0), _p(dzr), zstride, rows, K, G, F, st),
                      'taps_backward_data')
                # dX += dz0 + A(dz1 + A(dz2 + ... A dz_{K-1}))   with A = adjoint shift = CSR(S_e) SpMM
                for k in range(K - 1, 0, -1):
                    dst = dzr[k - 2] if k >= 2 else dz0
                    spmm_raw(graph.adj[e], dzr[k - 1], out=dst, accumulate=True)
                dX = dz0 if dX is None else dX.add_(dz0)
            if need_w or need_b:
                # per-split partial sums, added in a fixed order: the weight gradient is bit-reproducible
                nsp, nbb = C.c_int64(0), C.c_int64(0)
                check(lib.gcrnn_taps_backward_weight_parts(rows, K, G, F, C.byref(nsp), C.byref(nbb)), 'taps_backward_weight_parts')
                dwp = torch.empty((nsp.value, F, K, G), dtype=X.dtype, device=X.device)
                dbp = torch.empty((nbb.value, F), dtype=X.dtype, device=X.device) if (need_b and e == 0) else None
                check(lib.gcrnn_taps_backward_weight(dt, _p(dy), _p(X), _p(zrest[e]) if K > 1 else None, zstride,
                                                     _p(dwp), _p(dbp), ctx.bias_scale, rows, K, G, F, st), 'taps_backward_weight')
                if need_w:
                    if E == 1:
                        dW = dwp.sum(dim=0).view(F, 1, K, G)
                    else:
                        dW[:, e] = dwp.sum(dim=0)
                if dbp is not None:
                    db = dbp.sum(dim=0)
        if db is not None:
            db = db.view(ctx.bias_shape)
        return dX, dW, db, None, None


def lsigf_node_major(X, w, bias, graph, bias_scale=1.0):
    """X: [T][N][B][G] node-major -> [T][N][B][F]; w: F x E x K x G; bias: F x 1 or None."""
    require_device(X, w, bias)
    if w.dtype != X.dtype:
        raise GcrnnError('filter taps are %s but the signal is %s' % (w.dtype, X.dtype))
    if X.dtype == torch.bfloat16:
        # the any-shape filter kernels are fp32 / fp64 (bf16 lives in the cell's own kernels): a stand-alone bf16 filter is evaluated in fp32 and
        # rounded once at the end -- differentiable, the casts' backward returns bf16 gradients
        y = _LSIGF.apply(X.float(), w.float(), bias.float() if bias is not None else None, graph, bias_scale)
        return y.to(torch.bfloat16)
    return _LSIGF.apply(X, w, bias, graph, bias_scale)


# ------------------------------------------------------------------------------------------ fused flagship path
def fused_padded_inputs(F, G):
    """Input-feature count the fused kernels run with for a cell with G input and F state features: the x operand is
    consumed in 32-feature MFMA steps, so G is zero-padded to 32 (or 64) channels -- the reference drivers' G = 1
    (kStepPredGRNNs.py:220, epicenterEstimation.py:170) runs as 32. None: no kernel for this pair."""
    if F in (32, 64) and 0 < G <= 32:
        return 32
    if F == 64 and 32 < G <= 64:
        return 64
    return None


def fused_pad_operands(X, wA):
    """Zero-pad the input sequence X [B][T][G][N] and the input taps wA [F][1][K][G] to the kernels' channel count
    (differentiable w.r.t. wA: the padding's gradient is dropped by autograd)."""
    F, G = wA.shape[0], wA.shape[3]
    Gp = fused_padded_inputs(F, G)
    if Gp == G:
        return X, wA
    B, T, _, N = X.shape
    Xp = X.new_zeros((B, T, Gp, N))
    Xp[:, :, :G] = X
    return Xp, torch.nn.functional.pad(wA, (0, Gp - G))


def fused_supported(N, F, G, Kin, Kst, dtype, E=1):
    Gp = fused_padded_inputs(F, G)
    return (E == 1 and dtype == torch.bfloat16 and Gp is not None and
            bool(lib.gcrnn_fused_supported(int(N), int(F), int(Gp), int(max(Kin, Kst)))))


def time_fused_step_kernel(X, h0, wA, wB, bias, graph, reps=3, inline=None, user_layout=True, warm=1):
    """Average duration of ONE fused step launch, measured with HIP events on the launch stream
    (inputs pre-packed, only the T step launches sit between the events; on uniform-weight graphs each launch also lays out
    x_{t+1}, exactly as in fused_cell_forward). warm: untimed launches queued in front of the timed ones without a gap (behind an idle
    period the chip runs its first ~30 ms of load 10-25 % slower than its steady state, profiles/r04_clock_transient.txt)."""
    X, wA = fused_pad_operands(X, wA.detach())
    B, T, G, N = X.shape
    F = wA.shape[0]
    Kin, Kst = wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan()
    npad = plan['npad']
    st = _stream()
    dev = X.device
    xs = torch.empty((T, B, npad, G), dtype=torch.bfloat16, device=dev)
    h0s = torch.empty((1, B, npad, F), dtype=torch.bfloat16, device=dev)
    hs = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=dev)
    Xc, h0c = X.contiguous(), h0.contiguous()      # named: a temporary would be freed (and reusable) before the launch
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(Xc), _p(xs), B, T, G, N, npad, None, st), 'pack_seq')
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(h0c), _p(h0s), B, 1, F, N, npad, None, st), 'pack_seq')
    wpack = torch.empty(((F // 16) * K * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
    wAc, wBc = wA.contiguous(), wB.contiguous()
    check(lib.gcrnn_fused_pack_weights(dtype_code(wA.dtype), _p(wAc), _p(wBc), _p(wpack),
                                       F, G, Kin, Kst, st), 'pack_weights')
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    # same launch configuration as fused_cell_forward: the kernel also writes the user-layout output when it can
    # (user_layout=False: sequence-major in and out only -- what GGCRNNCell.forward_native issues)
    H = torch.empty((B, T, F, N), dtype=torch.bfloat16, device=dev) if (N % 8 == 0 and user_layout) else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ok = fused_inline_pack_ok(plan, N, F, G, K)          # the launches as the forward issues them: with the inline pack of x_{t+1} where it
    inline_arg = inline
    inline = (ok if inline is None else (ok and inline)) and X.data_ptr() % 16 == 0     # applies; inline=False times the bare step for comparison
    plan16 = fused_img16_plan(graph, False, None)
    wide = fused_wide_plan(graph, B, T, N, F, G, K, inline)
    if wide is None and plan16 is None:                  # rank-1-weighted graph (normalised adjacency): the wide kernel on the pattern plan, as fused_cell_forward issues it
        inl1 = inline_arg is not False and not os.environ.get('GCRNN_NO_INLINE_PACK') and X.data_ptr() % 16 == 0
        wide = fused_wide_plan(graph, B, T, N, F, G, K, inl1, rank1=True)
        if wide is None and inl1:
            inl1 = False
            wide = fused_wide_plan(graph, B, T, N, F, G, K, False, rank1=True)
        if wide is not None:
            inline = inl1
    if wide is not None:
        # the wide sequence-resident kernel (what fused_cell_forward issues for this problem): ONE launch per forward
        wpw = _fused_pack_weights_wide(wAc, wBc, wide['uniform_w'], st)
        scr = fused_state_scratch(wide, B, F, dev) if H is not None else None      # the launch the module issues under no_grad: no state image
        # ... and with the inline pack the self-start form, which reads the user-layout X and h0 itself (fused_cell_forward's dispatch)
        user16 = fused_wide_user_plan(graph, Xc, h0c, F, G, K) if (H is not None and scr is not None and inline) else None
        for rep in range(reps + warm):
            if rep == warm:
                e0.record()                              # (no synchronisation here: the timed launches follow the warm ones without an idle gap)
            if user16 is not None:
                _fused_forward_wide_user(user16, Xc, h0c, wAc, wBc, None, F, G, K, st, out=H, packs=(wpw, b32), buffers=(xs.view(torch.uint8).view(-1), scr))
                continue
            _fused_forward_wide(wide, xs, h0s, hs, wAc, wBc, b32, B, T, N, F, G, K, H, False, Xc if inline else None, st, wpw=wpw, scratch=scr)
        e1.record()
        torch.cuda.synchronize()
        per_step = 1e3 * e0.elapsed_time(e1) / (reps * T)
        return {'avg_us': per_step, 'launches': reps, 'inline_pack': bool(inline), 'steps_per_launch': T,
                'launch_avg_us': per_step * T, 'kernel': 'fused_seq32_kernel'}
    for rep in range(reps + 1):
        if rep == 1:                                     # (launch 0 is a warm-up: first touch of the fresh output buffers, code and plan not yet in cache)
            torch.cuda.synchronize()
            e0.record()
        check(lib.gcrnn_fused_forward_bf16(_p(xs), _p(h0s), _p(hs), _p(wpack), _p(b32), None, None, *_fused_graph_args(plan16 or plan),
                                           B, T, N, F, G, K, _p(H) if H is not None else None, 2 if plan16 else 0, None, plan.get('uniform_w', 0.0),
                                           _p(Xc) if inline else None, None, None, st),
              'fused_forward')
    e1.record()
    torch.cuda.synchronize()
    # time steps one launch covers: T on the sequence-resident persistent kernel (gcrnn_fused_seq.h), else 1 (one launch per step)
    spl = int(lib.gcrnn_fused_seq_steps_per_launch(B, T, N, F, G, K, int((plan16 or plan)['entries']), float(plan.get('uniform_w', 0.0)),
                                                   1 if plan16 else 0, 1 if inline else 0, 0))
    per_step = 1e3 * e0.elapsed_time(e1) / (reps * T)
    return {'avg_us': per_step, 'launches': reps * T // max(spl, 1), 'inline_pack': bool(inline), 'steps_per_launch': max(spl, 1),
            'launch_avg_us': per_step * max(spl, 1), 'kernel': 'fused_seq_kernel' if spl else 'fused_step_kernel'}


_PACK_CACHE = {}
_PARAM_EPOCH = [0]
_PACK_CACHE_ON = [bool(os.environ.get('GCRNN_PACK_CACHE'))]


def parameters_changed():
    """Tell the (opt-in) pack cache that parameters were written through a path PyTorch does not see: a kernel that updates them through raw
    pointers (optim.FlatAdam's flat Adam step, a replayed hipGraph of a whole training step) leaves their autograd version counters where they
    were. Every such writer calls this; the epoch is part of every key. Without `freeze_parameters()` nothing is cached and this is a no-op."""
    _PARAM_EPOCH[0] += 1


def freeze_parameters(on=True):
    """Opt in to (or out of) keeping the PACKED forms of parameters -- tap fragments, the fp32 bias, concatenated gate weights -- between
    forwards. The default is OFF: every forward packs from the live parameters (three ~5 us kernels, ~1 % of a forward at the bench size), so
    ANY write PyTorch permits is seen by the next forward -- including `p.data.mul_(2)`, `p.data.copy_(t)` and `dist.broadcast(p.data, 0)`,
    which move no version counter the host could key on (the reference's own `reset_parameters`, Utils/graphML.py:2229-2235, writes that way).
    With the cache on the caller promises not to write parameters through `.data` or raw pointers without calling `parameters_changed()`;
    in-place updates under `torch.no_grad()`, `copy_`, `load_state_dict` and tensor swaps are still detected (storage pointer + version
    counter in the key). GCRNN_PACK_CACHE=1 in the environment switches it on from the start. Returns the previous setting."""
    prev = _PACK_CACHE_ON[0]
    _PACK_CACHE_ON[0] = bool(on)
    if not on:
        _PACK_CACHE.clear()
    return prev


class frozen_parameters(object):
    """`with ops.frozen_parameters(): ...` -- freeze_parameters(True) for the block (an inference loop over fixed weights)."""

    def __enter__(self):
        self._prev = freeze_parameters(True)
        return self

    def __exit__(self, *exc):
        freeze_parameters(self._prev)
        return False


def _cached_pack(kind, tensors, extra, st, make):
    """Packed forms of PARAMETERS (tap fragments, the fp32 bias). DEFAULT: made on every call from the live parameters -- correct for every
    way PyTorch lets a parameter be written (see freeze_parameters). With `freeze_parameters()` / GCRNN_PACK_CACHE=1 they are kept between
    calls while the parameters are unchanged: the key holds each tensor's storage pointer, shape, strides, dtype and autograd version counter
    plus the parameter epoch, and the entry keeps the tensors alive so that their storage cannot be recycled under the key. Never during a
    stream capture: a miss there would store a buffer whose pack kernel was only RECORDED, and a second capture of the same cell would hit it
    and record no pack at all (its replays would read memory another graph fills) -- every captured graph packs for itself, so its replays
    always see the live weights. Temporaries made under torch.inference_mode (no version counter) are never cached."""
    if (not _PACK_CACHE_ON[0] or os.environ.get('GCRNN_NO_PACK_CACHE') or torch.cuda.is_current_stream_capturing()
            or any(t.is_inference() for t in tensors)):
        return make()
    key = (kind, extra, st.value, _PARAM_EPOCH[0]) + tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) for t in tensors)
    hit = _PACK_CACHE.get(key)
    if hit is not None:
        return hit[0]
    out = make()
    while len(_PACK_CACHE) >= 64:
        _PACK_CACHE.pop(next(iter(_PACK_CACHE)))
    _PACK_CACHE[key] = (out, tensors)
    return out


def _bias_f32(bias, st):
    """[F] fp32 copy of the bias (or None), cached while the parameter is unchanged."""
    if bias is None:
        return None
    b = bias.detach()
    if b.dtype == torch.float32 and b.is_contiguous():
        return b.view(-1)
    return _cached_pack('bias', (b,), None, st, lambda: b.float().contiguous().view(-1))


def _fused_pack_weights(wA, wB, st):
    F, G = wA.shape[0], wA.shape[3]
    Kin, Kst = wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)

    def make():
        wpack = torch.empty(((F // 16) * K * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=wA.device)
        wAc, wBc = wA.contiguous(), wB.contiguous()
        check(lib.gcrnn_fused_pack_weights(dtype_code(wA.dtype), _p(wAc), _p(wBc), _p(wpack),
                                           F, G, Kin, Kst, st), 'pack_weights')
        return wpack
    return _cached_pack('taps16', (wA.detach(), wB.detach()), None, st, make)


def _fused_pack_weights_wide(wA, wB, uniform_w, st):
    """Taps as the MFMA A fragments of the wide sequence-resident kernel (csrc/gcrnn_fused_seq32.h): 32-feature chunks, feature
    permutation of the rows, tap k scaled by uniform_w^k. wA [Fout][1][Kin][G], wB [Fout][1][Kst][F]: Fout = F for a cell, 2 F for the
    two time gates' sub-cells stacked over their output features."""
    Fout, G, F = wA.shape[0], wA.shape[3], wB.shape[3]
    Kin, Kst = wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)

    def make():
        wpack = torch.empty(((Fout // 32) * K * 2 * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=wA.device)
        wAc, wBc, kin = wA.contiguous(), wB.contiguous(), Kin
        if G == 0:                                   # state-only operand (the BPTT chain's transposed taps): no input taps to read
            wAc, kin = wBc, Kst
        check(lib.gcrnn_fused_pack_weights_wide(dtype_code(wB.dtype), _p(wAc), _p(wBc), _p(wpack), Fout, F, G, kin, Kst, float(uniform_w), st),
              'pack_weights_wide')
        return wpack
    return _cached_pack('taps32', (wA.detach(), wB.detach()), float(uniform_w), st, make)


def _fused_pack_weights_wide_bias(wA, wB, bias, uniform_w, st):
    """_fused_pack_weights_wide of a cell's taps together with the fp32 copy of its bias [F], written by the SAME launch
    (gcrnn_fused_pack_weights_wide_bias): (wpack, b32). Kept under the live-parameter rule of _cached_pack like the two it replaces. A bias
    of another dtype than the taps (or none) takes the two separate packs."""
    if bias is None or bias.dtype != wB.dtype or wA.dtype != wB.dtype:
        return _fused_pack_weights_wide(wA, wB, uniform_w, st), _bias_f32(bias, st)
    Fout, G, F = wA.shape[0], wA.shape[3], wB.shape[3]
    Kin, Kst = wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    b = bias.detach()
    assert b.numel() == Fout and G > 0

    def make():
        wpack = torch.empty(((Fout // 32) * K * 2 * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=wA.device)
        b32 = torch.empty((Fout,), dtype=torch.float32, device=wA.device)
        wAc, wBc, bc = wA.contiguous(), wB.contiguous(), b.contiguous()
        check(lib.gcrnn_fused_pack_weights_wide_bias(dtype_code(wB.dtype), _p(wAc), _p(wBc), _p(bc), _p(wpack), _p(b32), Fout, F, G, Kin, Kst,
                                                     float(uniform_w), st), 'pack_weights_wide_bias')
        return wpack, b32
    return _cached_pack('taps32b', (wA.detach(), wB.detach(), b), float(uniform_w), st, make)


def fused_wide_user_plan(graph, X, h0, F, G, K, head=False):
    """The bf16-image plan (uniform-weight or rank-1) when the SELF-START form of the wide inference forward takes the problem (the launch
    reads the user-layout h0 and X itself: no layout launch in front of it; csrc/gcrnn_fused_seq32.h), else None. X [B][T][G][N],
    h0 [B][F][N]: contiguous bf16, 16-byte aligned, N % 8 == 0, F and G multiples of 32; every T >= 1 (T <= 2 included: the form needs
    no caller-packed x_1) and every B (one workgroup per sequence). head: the output-head launch's form. GCRNN_SEQ32_SELF_START=0 (read by the library at every call) and GCRNN_NO_INLINE_PACK=1 switch it off."""
    B, T, _, N = X.shape
    if (os.environ.get('GCRNN_NO_INLINE_PACK') or X.dtype != torch.bfloat16 or h0.dtype != torch.bfloat16 or X.shape[2] != G
            or not X.is_contiguous() or not h0.is_contiguous() or X.data_ptr() % 16 or h0.data_ptr() % 16 or N % 8 or F % 32 or G % 32):
        return None
    plan16 = _forward_plan16(graph)
    if plan16 is None:
        plan16 = _forward_plan16(graph, rank1=True)
    if plan16 is None:
        return None
    query = lib.gcrnn_fused_forward_wide_head_user_supported if head else lib.gcrnn_fused_forward_wide_user_supported
    ok = query(int(B), int(T), int(N), int(F), int(G), int(K), int(plan16['entries']), float(plan16.get('uniform_w', 0.0)),
               3 if plan16.get('rank1') else 1)
    return plan16 if ok else None


_WIDE_SELF_START = 2      # GCRNN_WIDE_SELF_START (include/gcrnn.h): bit 1 of gcrnn_fused_forward_wide_scratch_bf16's huser_last_only


def _fused_forward_wide_user(plan16, X, h0, wA, wB, bias, F, G, K, st, last_only=False, out=None, packs=None, buffers=None, head=None):
    """ONE weight + bias pack launch and ONE launch of the wide kernel's self-start form on the user-layout X and h0 -- issued through
    gcrnn_fused_forward_wide_scratch_bf16 with GCRNN_WIDE_SELF_START (the un-gated inference forward is one call of that entry point
    whichever way its inputs are laid out; gcrnn_fused_forward_wide_user_bf16 is the same launch for C callers). Returns H [B][T or 1][F][N]
    bf16 -- or, head = (hw [F] fp32, hb [1] fp32 or None), y [B][T][N] fp32 from gcrnn_fused_forward_wide_head_user_bf16. The work buffer and the scratch are allocated per call on the current stream (two forwards on two streams never share them)
    unless the caller brings its own (buffers = (work, scratch))."""
    B, T, _, N = X.shape
    dev = X.device
    if buffers is not None:
        work, scr = buffers
    else:
        scr = fused_state_scratch(plan16, B, F, dev)
        work = torch.empty((int(lib.gcrnn_fused_forward_wide_user_bytes(int(B), int(T), int(G))),), dtype=torch.uint8, device=dev)
    assert scr is not None
    wpw, b32 = packs if packs is not None else _fused_pack_weights_wide_bias(wA.detach(), wB.detach(), bias, plan16['uniform_w'], st)
    if head is not None:
        hw, hb = head
        if out is None:
            out = torch.empty((B, T, N), dtype=torch.float32, device=dev)
        else:
            assert out.dtype == torch.float32 and out.device == dev and tuple(out.shape) == (B, T, N) and out.is_contiguous(), 'out: contiguous fp32 [B][T][N]'
        check(lib.gcrnn_fused_forward_wide_head_user_bf16(_p(work), int(work.numel()), _p(h0), _p(scr), int(scr.numel()), _p(wpw), _p(b32),
                                                          *_wide_graph_args(plan16), B, T, N, F, G, K, _p(hw), _p(hb), _p(out), _p(X),
                                                          _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
              'fused_forward_wide_head_user')
        return out
    H = out if out is not None else torch.empty((B, 1 if last_only else T, F, N), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_fused_forward_wide_scratch_bf16(_p(work), _p(h0), _p(scr), int(scr.numel()), _p(wpw), _p(b32), None, None,
                                                    *_wide_graph_args(plan16), B, T, N, F, G, K, _p(H),
                                                    int(bool(last_only)) | _WIDE_SELF_START, _p(X),
                                                    _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
          'fused_forward_wide_scratch (self-start)')
    return H


def fused_wide_plan(graph, B, T, N, F, G, K, inline, rank1=False, gated=False):
    """The bf16-image plan when the wide sequence-resident kernel (gcrnn_fused_forward_wide_bf16: un-gated forward as ONE launch, 32-feature
    chunks) takes this problem, else None. GCRNN_SEQ32=0 switches it off (A/B)."""
    plan16 = _forward_plan16(graph)
    if plan16 is None and rank1:
        plan16 = _forward_plan16(graph, rank1=True)
    if plan16 is None or F % 32 or G % 32:
        return None
    ok = lib.gcrnn_fused_forward_wide_supported(int(B), int(T), int(N), int(F), int(G), int(K), int(plan16['entries']),
                                                float(plan16.get('uniform_w', 0.0)), (3 if plan16.get('rank1') else 1) | (4 if gated else 0), 1 if inline else 0)
    return plan16 if ok else None


def fused_state_scratch(plan16, B, F, dev):
    """The scratch of the wide forward WITHOUT a state image (gcrnn_fused_forward_wide_scratch_bf16: inference through the user-layout H -- the
    launch keeps only what it re-reads itself, chunks 0 .. F/32-2 of h_t in slot order, 64 KB per workgroup at F = 64), or None when that form
    does not take the problem (split batch, GCRNN_SEQ32_STATE_SCRATCH=0, GCRNN_SEQ32P=1: the caller passes hs). Allocated per forward on the
    current stream, like hs: two forwards on two streams never share one."""
    need = int(lib.gcrnn_fused_forward_wide_scratch_bytes(int(B), int(F), 1 if plan16.get('rank1') else 0))
    if need < 0:
        return None
    return torch.empty((need,), dtype=torch.uint8, device=dev)


def _fused_forward_wide(plan16, xs, h0s, hs, wA, wB, b32, B, T, N, F, G, K, H, last_only, Xinline, st, wpw=None, gi=None, gf=None, scratch=None):
    if wpw is None:
        wpw = _fused_pack_weights_wide(wA.detach(), wB.detach(), plan16['uniform_w'], st)
    if scratch is not None:                              # no state image: hs is not touched (and need not exist)
        assert H is not None
        check(lib.gcrnn_fused_forward_wide_scratch_bf16(_p(xs), _p(h0s), _p(scratch), int(scratch.numel()), _p(wpw), _p(b32), _p(gi), _p(gf),
                                                        *_wide_graph_args(plan16), B, T, N, F, G, K,
                                                        _p(H), int(bool(last_only)), _p(Xinline) if Xinline is not None else None,
                                                        _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
              'fused_forward_wide_scratch')
        return
    check(lib.gcrnn_fused_forward_wide_bf16(_p(xs), _p(h0s), _p(hs), _p(wpw), _p(b32), _p(gi), _p(gf),
                                            *_wide_graph_args(plan16), B, T, N, F, G, K,
                                            _p(H) if H is not None else None, int(bool(last_only)), _p(Xinline) if Xinline is not None else None,
                                            _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
          'fused_forward_wide')


def _wide_head_plan(graph, B, T, N, F, G, K, inline, gated=False):
    """The bf16-image plan (uniform-weight or rank-1) when the wide kernel's head variant (gcrnn_fused_forward_wide_head_bf16: cell + output
    head Linear(F -> 1) as ONE launch on the state scratch) takes this problem, else None."""
    if gated and inline:
        return None
    plan16 = _forward_plan16(graph)
    if plan16 is None:
        plan16 = _forward_plan16(graph, rank1=True)
    if plan16 is None or F % 32 or G % 32:
        return None
    ok = lib.gcrnn_fused_forward_wide_head_supported(int(B), int(T), int(N), int(F), int(G), int(K), int(plan16['entries']),
                                                     float(plan16.get('uniform_w', 0.0)), (3 if plan16.get('rank1') else 1) | (4 if gated else 0),
                                                     1 if inline else 0)
    return plan16 if ok else None


def fused_wide_head_supported(graph, B, T, N, F, G, K, gated=False):
    """True when cell + output head Linear(F -> 1) runs as ONE launch of the wide sequence-resident kernel (fused_cell_forward_wide_head;
    csrc/gcrnn_fused_seq32.h VAR bit 3) at this shape: what the wide forward on the state scratch takes -- uniform-weight and rank-1-weighted
    graphs, batches that are not split, F and G (padded) multiples of 32. gated: the time-gated cell."""
    return _wide_head_plan(graph, B, T, N, F, G, K, False, gated=gated) is not None


def _fused_forward_wide_head(plan16, xs, h0s, wA, wB, b32, B, T, N, F, G, K, hw, hb, Xinline, st, gi=None, gf=None, out=None):
    """ONE launch: the recurrence with the head in its epilogue. Returns y [B][T][N] fp32 (`out`, or a fresh tensor). The scratch is allocated
    per call on the current stream, as fused_state_scratch's callers do."""
    dev = xs.device
    scr = fused_state_scratch(plan16, B, F, dev)
    assert scr is not None
    if out is None:
        out = torch.empty((B, T, N), dtype=torch.float32, device=dev)
    else:
        assert out.dtype == torch.float32 and out.device == dev and tuple(out.shape) == (B, T, N) and out.is_contiguous(), 'out: contiguous fp32 [B][T][N]'
    wpw = _fused_pack_weights_wide(wA.detach(), wB.detach(), plan16['uniform_w'], st)
    check(lib.gcrnn_fused_forward_wide_head_bf16(_p(xs), _p(h0s), _p(scr), int(scr.numel()), _p(wpw), _p(b32), _p(gi), _p(gf),
                                                 *_wide_graph_args(plan16), B, T, N, F, G, K, _p(hw), _p(hb), _p(out),
                                                 _p(Xinline) if Xinline is not None else None,
                                                 _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
          'fused_forward_wide_head')
    return out


def fused_cell_forward_wide_head(X, h0, wA, wB, bias, graph, head, gates=None, gate_values=None, out=None, self_start=False):
    """Inference of cell + output head as ONE launch of the wide kernel (fused_cell_forward's arguments; head = (weight 1 x F, bias [1] or
    None)): y B x T x 1 x N fp32, a view of the [B][T][N] array the kernel writes -- `out`, when given (contiguous fp32 [B][T][N]). Raises where
    fused_wide_head_supported says no; GCRNN_NO_WIDE_HEAD does not apply here (it switches the DISPATCH of fused_cell_forward off)."""
    if self_start:
        # the launch reads the user-layout X and h0 itself (gcrnn_fused_forward_wide_head_user_bf16): no layout launch in front of it. Opt-in:
        # the dispatch of fused_cell_forward(head=...) -- the regression model's forward -- is pinned by its launch-count tests to ONE call
        # of gcrnn_fused_forward_wide_head_bf16, whose argument list has no room for the switch. Bit-identical y.
        assert gates is None and gate_values is None, 'self_start: the un-gated cell'
        return fused_cell_forward(X, h0, wA, wB, bias, graph, head=head, _head_out=out, _head_wide='self_start')
    return fused_cell_forward(X, h0, wA, wB, bias, graph, gates=gates, gate_values=gate_values, head=head, _head_out=out, _head_wide='require')


def _forward_plan16(graph, rank1=False):
    """The bf16-image plan of the forward graph (GraphOperator.fused_plan_img16: uniform-weight graphs only) or, with rank1, the plan of a
    rank-1-weighted graph (normalised adjacency): the plan of its 0/1 pattern + the two factor tables. None where the graph has no such
    plan; GCRNN_NO_IMG16=1 switches both off (A/B, and the fp32-image tests)."""
    if os.environ.get('GCRNN_NO_IMG16'):
        return None
    return graph.fused_plan_rank1() if rank1 else graph.fused_plan_img16()


def _adjoint_plan16(graph, rank1=False):
    """_forward_plan16 for the adjoint graph (S^T, the BPTT's hops; rank1: the adjoint plan of the pattern + the swapped factors)."""
    if os.environ.get('GCRNN_NO_IMG16'):
        return None
    return graph.fused_plan_rank1(adjoint=True) if rank1 else graph.fused_plan_img16(adjoint=True)


def _fused_forward_steps(graph, xs, h0s, hs, wpack, b32, B, T, N, F, G, K, H, last_only, Xinline, st, gi=None, gf=None, evs=None, hw=None, part=None):
    """The forward on the 16-feature step kernel (gcrnn_fused_forward_bf16; the launcher beside _fused_forward_wide). H: the user-layout
    output the launches store themselves, or None; hw / part: the fused head's weights and its partial sums."""
    plan = graph.fused_plan()
    plan16 = _forward_plan16(graph)
    check(lib.gcrnn_fused_forward_bf16(_p(xs), _p(h0s), _p(hs), _p(wpack), _p(b32), _p(gi), _p(gf), *_fused_graph_args(plan16 or plan),
                                       B, T, N, F, G, K, _p(H), int(bool(last_only)) | (2 if plan16 else 0), evs, plan.get('uniform_w', 0.0),
                                       _p(Xinline), _p(hw), _p(part), st), 'fused_forward')


def fused_img16_plan(graph, gated, head):
    """The bf16-image plan of the un-gated forward steps, or None (_forward_plan16; un-gated and time-gated cells, with or without the
    fused head)."""
    return _forward_plan16(graph)


def _fused_graph_args(plan):
    return (_p(plan['tile_slots']), _p(plan['tile_off']), _p(plan['ell_addr']), _p(plan['ell_val']),
            _p(plan['ell_val4']), _p(plan['ell_col4']), plan['entries'])


def _wide_graph_args(plan16):
    return _p(plan16['tile_slots']), _p(plan16['tile_off']), _p(plan16['ell_col4']), plan16['entries']


_SIDE_STREAMS = {}


def _side_stream(dev):
    s = _SIDE_STREAMS.get(dev)
    if s is None:
        s = _SIDE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return s


def fused_inline_pack_ok(plan, N, F, G, K):
    """The step kernel can lay out x_{t+1} itself (gcrnn_fused_forward_bf16 with Xuser_inline): uniform-weight graph image with LDS
    room for the input tile, N % 8 == 0. GCRNN_NO_INLINE_PACK=1 switches it off (A/B)."""
    if os.environ.get('GCRNN_NO_INLINE_PACK'):
        return False
    return bool(lib.gcrnn_fused_inline_pack_supported(int(N), int(F), int(G), int(K), int(plan['entries']), float(plan.get('uniform_w', 0.0))))


def fused_pad_taps(wA):
    """Input taps wA [F][1][K][G] zero-padded to the kernels' input width (differentiable; see fused_pad_operands)."""
    F, G = wA.shape[0], wA.shape[3]
    Gp = fused_padded_inputs(F, G)
    return wA if Gp == G else torch.nn.functional.pad(wA, (0, Gp - G))


def _pad_tap_count(w, K):
    """Taps w [F][1][k][C] with zero taps appended up to K of them."""
    k = w.shape[2]
    return w if k == K else torch.cat([w, w.new_zeros(w.shape[0], 1, K - k, w.shape[3])], dim=2)


def _transposed_taps(w):
    """Taps w [F_out][1][K][F_in] -> [F_in][1][K][F_out]: the adjoint filter's (detached)."""
    return w.detach()[:, 0].permute(2, 1, 0).contiguous().unsqueeze(1)


def _pad_gate_inputs(wA_g, G):
    """A gate sub-cell's input taps [F][1][K][g] with zero taps for the padded input channels (g < G = 32)."""
    return wA_g if wA_g.shape[3] == G else torch.nn.functional.pad(wA_g.detach(), (0, G - wA_g.shape[3]))


def _unpack_states(hs, H, last_only, N, st):
    """The states hs [T][B][NPad][F] (the last one alone with last_only) into the user-layout H, where the kernels could not store it
    themselves (N % 8 != 0: no 16-byte row stores)."""
    T, B, npad, F = hs.shape
    src = hs[T - 1:] if last_only else hs
    check(lib.gcrnn_unpack_seq_major(_lib.BF16, _p(src), _p(H), B, 1 if last_only else T, F, N, npad, None, st), 'unpack_seq')


def _unpack_grad(ds, B, T, C, N, st):
    """A sequence-major gradient ds [T][B][NPad][C] bf16 in the user layout, [B][T][C][N] bf16."""
    g = torch.empty((B, T, C, N), dtype=torch.bfloat16, device=ds.device)
    check(lib.gcrnn_unpack_seq_major(_lib.BF16, _p(ds), _p(g), B, T, C, N, ds.shape[-2], None, st), 'unpack_seq')
    return g


def fused_pack_inputs(X, h0, graph, overlap=False, first_only=False, channels=None, states=True):
    """user-layout bf16 X [B][T][G][N], h0 [B][F][N] -> sequence-major xs [T][B][NPad][G] and the state buffer
    hs_all [T+1][B][NPad][F] whose slot 0 holds h0 (slots 1..T receive h_1..h_T: hs_all[:T] is then the h_{t-1} operand of
    every step, which the gate-gradient pass reads as one array).
    overlap: only step 0 is packed on the current stream; every later step is packed on a side stream by a kernel small
    enough (4 KiB of LDS, bounded grid) to run beside the step kernels, each followed by an event. Returns (xs, hs_all,
    events) with events[t] = the event step t's launch has to wait for -- the recurrence starts after 1/T of the pack.
    states=False: hs_all is slot 0 alone (inference that may run without a state image, fused_state_scratch; a caller that turns out to
    need the image allocates it then)."""
    B, T, G, N = X.shape
    F = h0.shape[1]
    npad = graph.fused_plan()['npad']
    st = _stream()
    TS = T if states else 0
    Xc, h0c = X.contiguous(), h0.contiguous()
    if channels is not None and channels != G:
        # X keeps its own G channels in the user layout; the sequence-major array gets `channels` of them, the rest zeros
        assert channels > G and not overlap and not first_only
        xs = torch.empty((T, B, npad, channels), dtype=torch.bfloat16, device=X.device)
        hs_all = torch.empty((TS + 1, B, npad, F), dtype=torch.bfloat16, device=X.device)
        check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(h0c), _p(hs_all), B, 1, F, N, npad, None, st), 'pack_seq')
        check(lib.gcrnn_pack_seq_major_padded(_p(Xc), _p(xs), B, T, G, channels, N, npad, st), 'pack_seq_padded')
        return xs, hs_all
    xs = torch.empty((T, B, npad, G), dtype=torch.bfloat16, device=X.device)
    hs_all = torch.empty((TS + 1, B, npad, F), dtype=torch.bfloat16, device=X.device)
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(h0c), _p(hs_all), B, 1, F, N, npad, None, st), 'pack_seq')
    if first_only:                                       # x_0 and x_1 only: the step kernels lay out every later step themselves (inline pack;
        # the sequence-resident kernel works two steps ahead, the chunk-parallel one re-writes x_1 with the same bits)
        check(lib.gcrnn_pack_seq_major_steps(_p(Xc), _p(xs), B, T, G, N, npad, 0, min(2, T), 0, st), 'pack_seq_steps')
        return xs, hs_all
    if not overlap:
        check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(Xc), _p(xs), B, T, G, N, npad, None, st), 'pack_seq')
        return xs, hs_all
    main = torch.cuda.current_stream(X.device)
    side = _side_stream(X.device)
    check(lib.gcrnn_pack_seq_major_steps(_p(Xc), _p(xs), B, T, G, N, npad, 0, 1, 0, st), 'pack_seq_steps')
    ready = torch.cuda.Event()
    ready.record(main)                                   # X and the fresh buffers are valid on the main stream from here on
    side.wait_event(ready)
    events = [None] * T
    sst = C.c_void_p(side.cuda_stream)
    # one workgroup per CU walks the tiles of a step: measured on MI355X the side-stream pack of step t+1 then takes about as
    # long as step t (118 us vs 120 us at B = 256) and slows it by 9 %; an unbounded grid starves the step kernels of memory
    # bandwidth (steps 1.2x .. 3.2x slower: no net gain), half the grid makes the pack the bottleneck
    blocks = int(os.environ.get('GCRNN_PACK_BLOCKS', torch.cuda.get_device_properties(X.device).multi_processor_count))
    for t in range(1, T):
        check(lib.gcrnn_pack_seq_major_steps(_p(Xc), _p(xs), B, T, G, N, npad, t, t + 1, blocks, sst), 'pack_seq_steps')
        ev = torch.cuda.Event()
        ev.record(side)
        events[t] = ev
    Xc.record_stream(side)
    xs.record_stream(side)
    return xs, hs_all, events


class _PendingLayout(object):
    """The part of X that fused_pack_inputs_gated left to the first gate pre-pass: xs [T][B][NPad][G] holds its leading `steps` time steps,
    x_user is the user-layout tensor the rest comes from (None once settled). The cell entry points hand the object to their pre-passes
    (`pending=`) and check that it is settled before the recurrence reads xs."""

    def __init__(self, xs, x_user, steps):
        self.xs, self.x_user, self.steps = xs, x_user, steps

    @property
    def settled(self):
        return self.x_user is None

    def settle(self, consumer_steps):
        """The user-layout tensor a gate pre-pass should lay out while it runs, or None. The pending layout was sized for the pre-pass that
        was expected to run first; when another one runs instead -- it does not lay out at this shape (consumer_steps <= 0), or counts on a
        different number of leading steps -- the rest of X is laid out here, by the plain pack. Either way nothing is pending afterwards."""
        x_user, self.x_user = self.x_user, None
        if x_user is None or (consumer_steps > 0 and consumer_steps == self.steps):
            return x_user
        T, B, npad, G = self.xs.shape
        check(lib.gcrnn_pack_seq_major_steps(_p(x_user), _p(self.xs), B, T, G, x_user.shape[3], npad, self.steps, T, 0, _stream()), 'pack_seq_steps')
        return None


def fused_pack_inputs_gated(X, h0, graph, F, K, states=True):
    """fused_pack_inputs for a cell whose FIRST consumer of xs is a gate pre-pass (fused_time_gate): on a uniform-weight graph with
    a batch that fills the chip, only the first time step(s) are laid out here and that pre-pass lays out the rest while it runs
    (gcrnn_fused_gate_prepass_pack_bf16: every item packs the operand of its workgroup's next item) -- the 0.5 ms pass over X at
    B = 256, T = 32 goes away. Returns (xs, hs_all, pending): the _PendingLayout that pre-pass takes, or None when all of X is laid out."""
    B, T, G, N = X.shape
    plan = graph.fused_plan()
    plan16 = fused_img16_plan(graph, True, None)
    steps = 0
    if plan16 is not None and X.dtype == torch.bfloat16 and X.is_contiguous() and X.data_ptr() % 16 == 0 and not os.environ.get('GCRNN_NO_INLINE_PACK'):
        _, steps = fused_gate_pair_plan(graph, B, T, N, F, G, K, True)      # (the wide kernel's gate-pair pre-pass lays X out, when it takes the problem)
        if steps <= 0:
            steps = _gate_prepass_lays_out(plan, plan16, B, T, N, F, G, K)
    if steps <= 0 or steps >= T:
        return fused_pack_inputs(X, h0, graph, states=states) + (None,)
    xs, hs_all = _pack_leading_steps(X, h0, plan['npad'], F, steps, states)
    return xs, hs_all, _PendingLayout(xs, X, steps)


def _pack_leading_steps(X, h0, npad, F, steps, states=True):
    """fused_pack_inputs with only the first `steps` time steps of the contiguous X laid out: the first consumer of xs lays out the rest."""
    B, T, G, N = X.shape
    st = _stream()
    xs = torch.empty((T, B, npad, G), dtype=torch.bfloat16, device=X.device)
    hs_all = torch.empty(((T if states else 0) + 1, B, npad, F), dtype=torch.bfloat16, device=X.device)
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(h0.contiguous()), _p(hs_all), B, 1, F, N, npad, None, st), 'pack_seq')
    check(lib.gcrnn_pack_seq_major_steps(_p(X), _p(xs), B, T, G, N, npad, 0, steps, 0, st), 'pack_seq_steps')
    return xs, hs_all


def _gate_prepass_lays_out(plan, plan16, B, T, N, F, G, K):
    """The leading time steps of xs the 16-feature gate pre-pass counts on when it lays out X itself (0: it does not at this shape)."""
    if plan16 is None:
        return 0
    return int(lib.gcrnn_fused_gate_prepass_lays_out(B, T, N, F, G, K, plan16['entries'], plan.get('uniform_w', 0.0), 1))


def fused_overlap_ok(X):
    """The overlapped pack (opt-in: GCRNN_FUSED_OVERLAP=1) needs even N and G (4-byte accesses), more than one step, and no
    stream capture in progress. Off by default: measured on MI355X it gains 3 % when the two streams happen to share the CUs
    well (4.04 -> 3.90 ms per forward at B = 256) and loses up to 2x when they do not (same binary, another run) -- DESIGN 4.3."""
    B, T, G, N = X.shape
    return (T > 1 and N % 2 == 0 and G % 2 == 0 and os.environ.get('GCRNN_FUSED_OVERLAP', '0') == '1'
            and not torch.cuda.is_current_stream_capturing())


def fused_h0_zero_flag(h0):
    """int32 [1] on the device: 1 when the initial state is all zeros (every training loop of the reference starts from
    zeros(B, F, N), train_rnn.py:256). The gate kernels read it and skip the state operand's loads and matrix products -- a
    data-dependent short cut with bit-identical results, decided on the device (no host synchronisation)."""
    if h0.dtype == torch.bfloat16 and h0.is_contiguous() and h0.numel() % 8 == 0 and h0.data_ptr() % 16 == 0 and h0.is_cuda:
        flag = torch.empty(1, dtype=torch.int32, device=h0.device)
        check(lib.gcrnn_all_zero_flag_bf16(_p(h0), h0.numel(), _p(flag), _stream()), 'all_zero_flag')      # one pass at HBM rate, no temporaries
        return flag
    return (h0 == 0).all().to(torch.int32).view(1)


def fused_time_gate(xs, h0s, wA_g, wB_g, bias_g, lin_w, lin_b, graph, N, store_states=False, hzero=None, pending=None):
    """One time gate of the fused path for all (t, b) (graphML.py:2357-2374): sigmoid(Linear(vec(tanh(A_g(S)x_t + B_g(S)h0
    + 2 b_g)))) as ONE pre-pass launch. xs [T][B][NPad][G], h0s [1][B][NPad][F] sequence-major bf16. hzero: device int32
    flag (fused_h0_zero_flag), non-zero when h0 is all zeros -- the kernel then skips the state half of the operand. pending: the
    _PendingLayout of xs (fused_pack_inputs_gated), settled here. Returns the gate [T][B] fp32 (and, with store_states, the gate cell's states c [T][B][NPad][F] bf16 for its BPTT)."""
    T, B, npad, G = xs.shape
    F = wA_g.shape[0]
    K = max(wA_g.shape[2], wB_g.shape[2])
    plan = graph.fused_plan()
    st = _stream()
    wp = _fused_pack_weights(wA_g.detach(), wB_g.detach(), st)
    bg = bias_g.detach().float().contiguous().view(-1) if bias_g is not None else None
    gw = lin_w.detach().float().view(F, N).t().contiguous()                  # row-major vec over (f, n) -> [N][F]
    parts = torch.empty((T * B, (F // 16) * int(lib.gcrnn_fused_step_waves())), dtype=torch.float32, device=xs.device)
    cs = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=xs.device) if store_states else None
    plan16 = fused_img16_plan(graph, True, None)
    x_user = pending.settle(_gate_prepass_lays_out(plan, plan16, B, T, N, F, G, K)) if pending is not None else None
    if x_user is not None:
        # xs holds its first time step(s) only (fused_pack_inputs_gated): this pre-pass lays out the rest
        check(lib.gcrnn_fused_gate_prepass_pack_bf16(_p(x_user), _p(xs), _p(h0s), _p(wp), _p(bg), _p(gw), _p(parts), _p(cs),
                                                     *_fused_graph_args(plan16), B, T, N, F, G, K, _p(hzero), plan.get('uniform_w', 0.0),
                                                     1, st), 'gate_prepass_pack')
    else:
        check(lib.gcrnn_fused_gate_prepass_bf16(_p(xs), _p(h0s), _p(wp), _p(bg), _p(gw), _p(parts), _p(cs),
                                                *_fused_graph_args(plan16 or plan), B, T, N, F, G, K, _p(hzero), plan.get('uniform_w', 0.0),
                                                1 if plan16 else 0, st), 'gate_prepass')
    acc = parts.sum(dim=1)                                                    # fixed order: deterministic gates
    if lin_b is not None:
        acc = acc + lin_b.detach().float()
    gate = torch.sigmoid(acc).view(T, B).contiguous()
    return (gate, cs, gw) if store_states else gate


def _fused_time_gates_each(xs, h0s, gates, graph, N, hzero, pending=None):
    """(gi, gf) of fused_time_gate, one pre-pass launch per gate; the gates' input taps are padded to the channels of xs."""
    return tuple(fused_time_gate(xs, h0s, _pad_gate_inputs(g[0], xs.shape[3]), *g[1:], graph, N, hzero=hzero, pending=pending)
                 for g in (gates['in'], gates['forget']))


def fused_gate_pair_plan(graph, B, T, N, F, G, K, with_pack):
    """(plan16, steps) when the wide kernel's gate-PAIR pre-pass takes this problem (gcrnn_fused_gate_pair_prepass_wide_bf16: both time
    gates of every (t, b) in ONE launch), else (None, 0). steps: with_pack -- the leading time steps of xs the caller lays out itself."""
    plan16 = _forward_plan16(graph)
    if plan16 is None:
        plan16 = _forward_plan16(graph, rank1=True)
    if plan16 is None or F % 32 or G % 32 or os.environ.get('GCRNN_NO_GATE_PAIR'):
        return None, 0
    steps = int(lib.gcrnn_fused_gate_pair_wide_supported(int(B), int(T), int(N), int(F), int(G), int(K), int(plan16['entries']),
                                                         float(plan16.get('uniform_w', 0.0)), 3 if plan16.get('rank1') else 1, 1 if with_pack else 0))
    return (plan16, steps) if steps > 0 else (None, 0)


def fused_time_gate_pair(xs, h0s, gate_in, gate_f, graph, N, store_states=False, hzero=None, pending=None):
    """BOTH time gates of the fused path for all (t, b) (graphML.py:2357-2374) as ONE pre-pass launch of the wide sequence-resident kernel: the
    two sub-cells run as one cell of 2 F outputs, so an item's operand (x_t, h0) is loaded -- and, when xs still waits for its layout
    (pending: its _PendingLayout), laid out -- once. gate_* = (wA_g, wB_g, bias_g, lin_w, lin_b). Returns (gi, gf) [T][B] fp32, and with store_states
    also ((cs_in, gw_in), (cs_f, gw_f)): the sub-cells' states [T][B][NPad][F] bf16 and the read-out weights [N][F] fp32 for their BPTT."""
    T, B, npad, G = xs.shape
    F = gate_in[0].shape[0]
    K = max(gate_in[0].shape[2], gate_in[1].shape[2])
    st = _stream()
    x_user = pending.settle(fused_gate_pair_plan(graph, B, T, N, F, G, K, True)[1]) if pending is not None else None
    plan16, _ = fused_gate_pair_plan(graph, B, T, N, F, G, K, x_user is not None)
    assert plan16 is not None
    def prepare():      # everything derived from the gates' parameters alone: cached while they are unchanged (_cached_pack)
        wA2 = torch.cat([gate_in[0].detach(), gate_f[0].detach()], dim=0)
        wB2 = torch.cat([gate_in[1].detach(), gate_f[1].detach()], dim=0)
        wp_ = _fused_pack_weights_wide(wA2, wB2, plan16['uniform_w'], st)
        zb = torch.zeros(F, dtype=torch.float32, device=xs.device)
        b2_ = torch.cat([(g[2].detach().float().reshape(-1) if g[2] is not None else zb) for g in (gate_in, gate_f)]).contiguous()
        gws_ = [g[3].detach().float().view(F, N).t().contiguous() for g in (gate_in, gate_f)]      # row-major vec over (f, n) -> [N][F]
        lbs_ = [(g[4].detach().float() if g[4] is not None else None) for g in (gate_in, gate_f)]
        return wp_, b2_, gws_, torch.stack(gws_, dim=0).contiguous(), lbs_
    ptens = tuple(t.detach() for g in (gate_in, gate_f) for t in g if t is not None)
    wp, b2, gws, gw2, lbs = _cached_pack('gatepair', ptens, (float(plan16['uniform_w']), tuple(t is None for g in (gate_in, gate_f) for t in g)), st, prepare)
    nch = 2 * (F // 32)
    waves = int(lib.gcrnn_fused_step_waves())
    parts = torch.empty((T * B, nch * waves), dtype=torch.float32, device=xs.device)
    cs_in = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=xs.device) if store_states else None
    cs_f = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=xs.device) if store_states else None
    check(lib.gcrnn_fused_gate_pair_prepass_wide_bf16(_p(x_user), _p(xs), _p(h0s), _p(wp), _p(b2), _p(gw2), _p(parts), _p(cs_in), _p(cs_f),
                                                      *_wide_graph_args(plan16), B, T, N, F, G, K, _p(hzero), _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st), 'gate_pair_prepass')
    # read-out finish in ONE launch (round 5; until round 4 five torch launches): partials added in a fixed order, + bias, sigmoid
    out = [torch.empty((T, B), dtype=torch.float32, device=xs.device) for _ in range(2)]
    lbp = [(lb.reshape(-1).contiguous() if lb is not None else None) for lb in lbs]
    check(lib.gcrnn_gate_readout_finish(_p(parts), (nch // 2) * waves, _p(lbp[0]), _p(lbp[1]), _p(out[0]), _p(out[1]), T * B, st), 'gate_readout_finish')
    if store_states:
        return out[0], out[1], (cs_in, gws[0]), (cs_f, gws[1])
    return out[0], out[1]


def fused_cell_forward(X, h0, wA, wB, bias, graph, gates=None, return_states=False, gate_values=None, packed=None,
                       last_only=False, head=None, native_out=False, _head_out=None, _head_wide=None):
    """Whole GGCRNNCell forward (un-gated or time-gated) on the fused bf16 step kernel.

    X: B x T x G x N bf16, h0: B x F x N bf16 (user layout) -> H: B x T x F x N bf16.
    gates: None, or {'in': (wA_g, wB_g, bias_g, lin_weight [1, F*N], lin_bias), 'forget': (...)} -- the time-gate
    sub-networks GFL_* / MLP_* of the reference (graphML.py:2248-2278); each gate costs one pre-pass launch over all
    (t, b). gate_values: the two gates themselves, (gi, gf) [T][B] fp32, instead of their sub-networks. packed: the result
    of fused_pack_inputs (shared with the gates by the training path). No autograd graph is recorded here.
    return_states: also returns the state buffer hs_all [T+1][B][NPad][F] (slot 0 = h0) and the plan.
    last_only: H is B x 1 x F x N, the last state alone (the classification models' read-out); the user-layout store of the
    other steps is skipped.
    head: None, or (weight 1 x F, bias [1] or None) of an output head Linear(F -> 1) shared by all nodes (the regression model's
    `multipMlp` head with one output, architectures.py:1616-1627): it is evaluated in the epilogue of the wide sequence-resident kernel
    (ONE launch, fused_wide_head_supported; GCRNN_NO_WIDE_HEAD=1 switches that dispatch off) or else of the step kernel, H is never
    written in the user layout, and the function returns y: B x T x 1 x N (fp32) instead of H.
    native_out: H is returned as a VIEW of the sequence-major state image the recurrence keeps anyway (hs [T][B][NPad][F]:
    hs.permute(1, 0, 3, 2)[..., :N] has the reference's B x T x F x N shape, reference graphML.py:2425-2427) -- the launches skip the
    user-layout copy of every h_t (a third of the bytes they write); callers that need contiguity call .contiguous() themselves.
    """
    require_device(X, h0, wA, wB, bias)
    G0 = X.shape[2]                                      # (before any channel padding)
    if packed is None and X.shape[2] < wA.shape[3]:
        # taps already padded to the kernels' input width, X still with its own G channels (the drivers' G = 1): lay X out for the
        # kernels with the channel padding done by the pack itself -- no 32-channel copy of X in the user layout
        if X.shape[3] % 2 == 0 and X.dtype == torch.bfloat16:
            packed = fused_pack_inputs(X, h0, graph, channels=wA.shape[3])
        else:
            Xz = X.new_zeros((X.shape[0], X.shape[1], wA.shape[3], X.shape[3]))
            Xz[:, :, :X.shape[2]] = X
            X = Xz
    elif packed is None:
        X, wA = fused_pad_operands(X, wA.detach())        # G < 32: zero-padded input channels (no-op when already padded)
    B, T, _, N = X.shape
    G = wA.shape[3]
    F = wA.shape[0]
    K = max(wA.shape[2], wB.shape[2])
    plan = graph.fused_plan()
    st = _stream()
    dev = X.device
    X = X.contiguous()
    h0 = h0.contiguous()
    events = pending = None
    inline = False
    # inference through the user-layout H: the wide kernel then runs without a state image (fused_state_scratch) and hs is not allocated
    # here; a path that does need it allocates it below
    head_wide = head is not None and (_head_wide in ('require', 'self_start') or not os.environ.get('GCRNN_NO_WIDE_HEAD'))      # (the wide kernel's head variant may run)
    lean = packed is None and (head is None or head_wide) and not return_states and not native_out and N % 8 == 0
    if _head_wide == 'self_start':
        assert head is not None and lean and G0 == G and not last_only
        user16 = fused_wide_user_plan(graph, X, h0, F, G, K, head=True)
        if user16 is None:
            raise RuntimeError('fused_cell_forward_wide_head(self_start=True): the self-start head form does not take this problem')
        hw = head[0].detach().float().reshape(-1).contiguous()
        assert hw.numel() == F
        hb = head[1].detach().float().reshape(-1).contiguous() if head[1] is not None else None
        return _fused_forward_wide_user(user16, X, h0, wA, wB, bias, F, G, K, st, out=_head_out, head=(hw, hb)).unsqueeze(2)      # B x T x 1 x N (a view)
    if lean and head is None and gates is None and gate_values is None and G0 == G:
        # the wide kernel's self-start form: the launch reads the user-layout h0 and X itself -- no layout launch, no hs_all slot 0
        # (G < 32 keeps the channel-padding pack below; the output head's form is opt-in, fused_cell_forward_wide_head(self_start=True); GCRNN_SEQ32_SELF_START=0: the launches below, same binary)
        user16 = fused_wide_user_plan(graph, X, h0, F, G, K)
        if user16 is not None:
            return _fused_forward_wide_user(user16, X, h0, wA, wB, bias, F, G, K, st, last_only=last_only)
    if packed is not None:
        xs, hs_all = packed
    elif gates is None and gate_values is None and X.data_ptr() % 16 == 0 and (
            fused_inline_pack_ok(plan, N, F, G, K) or (head is None and not os.environ.get('GCRNN_NO_INLINE_PACK')
                                                       and fused_wide_plan(graph, B, T, N, F, G, K, True, rank1=True) is not None)
            or (head_wide and not os.environ.get('GCRNN_NO_INLINE_PACK') and _wide_head_plan(graph, B, T, N, F, G, K, True) is not None)):
        # un-gated cell on a uniform-weight graph: only x_0 is packed here, launch t lays out x_{t+1} itself (LDS-DMA into the room
        # the missing weight image leaves, read back transposed after the epilogue) -- no pack pass over X
        xs, hs_all = fused_pack_inputs(X, h0, graph, first_only=True, states=not lean)
        inline = True
    elif gates is None and fused_overlap_ok(X):          # (the gate pre-passes read every x_t at once: nothing to hide behind)
        xs, hs_all, events = fused_pack_inputs(X, h0, graph, overlap=True, states=not lean)
    elif gates is not None and gate_values is None:
        xs, hs_all, pending = fused_pack_inputs_gated(X, h0, graph, F, K, states=not lean)       # (the first gate pre-pass lays out x_1 .. x_{T-1})
    else:
        xs, hs_all = fused_pack_inputs(X, h0, graph, states=not lean)
    h0s, hs = hs_all[:1], hs_all[1:]
    gi = gf = None
    if gate_values is not None:
        gi, gf = (g.detach().float().contiguous() for g in gate_values)
        assert tuple(gi.shape) == (T, B) and tuple(gf.shape) == (T, B)
    elif gates is not None:
        hzero = fused_h0_zero_flag(h0)
        gp = {}
        for name in ('in', 'forget'):
            wA_g, wB_g, bias_g, lin_w, lin_b = gates[name]
            wA_g = _pad_gate_inputs(wA_g, G)
            assert max(wA_g.shape[2], wB_g.shape[2]) == K and wA_g.shape[0] == F
            gp[name] = (wA_g, wB_g, bias_g, lin_w, lin_b)
        pair16, _ = fused_gate_pair_plan(graph, B, T, N, F, G, K, pending is not None)
        if pair16 is not None:
            gi, gf = fused_time_gate_pair(xs, h0s, gp['in'], gp['forget'], graph, N, hzero=hzero, pending=pending)      # ONE launch for both gates
        else:
            gi, gf = _fused_time_gates_each(xs, h0s, gp, graph, N, hzero, pending)
    assert pending is None or pending.settled
    b32 = _bias_f32(bias, st)
    direct = (N % 8 == 0)                 # the step kernels write the user layout themselves (16-byte row stores)
    evs = None
    if events is not None:                               # raw hipEvent_t handles, one slot per step (host array, read during the call)
        evs = (C.c_void_p * T)(*[(e.cuda_event if e is not None else None) for e in events])
    if head is not None:
        assert not return_states and not last_only
        hw = head[0].detach().float().reshape(-1).contiguous()
        assert hw.numel() == F
        wide_h = _wide_head_plan(graph, B, T, N, F, G, K, inline, gated=(gi is not None)) if (head_wide and evs is None) else None
        if wide_h is not None:
            # ONE launch of the wide sequence-resident kernel: no state image, no per-step launches, y written as [B][T][N]
            hb = head[1].detach().float().reshape(-1).contiguous() if head[1] is not None else None
            y = _fused_forward_wide_head(wide_h, xs, h0s, wA, wB, b32, B, T, N, F, G, K, hw, hb, X if inline else None, st, gi=gi, gf=gf, out=_head_out)
            return y.unsqueeze(2)                                        # B x T x 1 x N (a view)
        if _head_wide == 'require':
            raise RuntimeError('fused_cell_forward_wide_head: the wide head form does not take this problem (fused_wide_head_supported)')
        if hs.shape[0] == 0:                             # (lean, and not the wide head form after all: the step kernels keep the state image)
            hs = torch.empty((T,) + tuple(h0s.shape[1:]), dtype=torch.bfloat16, device=dev)
        part = torch.empty((T, B, F // 16, N), dtype=torch.float32, device=dev)
        wpack = _fused_pack_weights(wA, wB, st)
        _fused_forward_steps(graph, xs, h0s, hs, wpack, b32, B, T, N, F, G, K, None, False, X if inline else None, st, gi, gf, evs, hw, part)
        y = part.sum(dim=2)                                          # fixed order over the F / 16 chunks
        if head[1] is not None:
            y = y + head[1].detach().float().reshape(())
        return y.permute(1, 0, 2).unsqueeze(2).contiguous()          # B x T x 1 x N
    wide = fused_wide_plan(graph, B, T, N, F, G, K, inline, rank1=True, gated=(gi is not None)) if (evs is None and head is None and not (gi is not None and inline)) else None
    if wide is not None:
        # un-gated cell, uniform-weight graph, a batch that fills the chip: ONE launch of the wide sequence-resident kernel
        if native_out:
            assert not return_states
            _fused_forward_wide(wide, xs, h0s, hs, wA, wB, b32, B, T, N, F, G, K, None, False, X if inline else None, st, gi=gi, gf=gf)
            Hv = hs.permute(1, 0, 3, 2)[:, :, :, :N]
            return Hv[:, T - 1:] if last_only else Hv
        H = torch.empty((B, 1 if last_only else T, F, N), dtype=torch.bfloat16, device=dev)
        scr = fused_state_scratch(wide, B, F, dev) if (direct and not return_states) else None
        if scr is None and hs.shape[0] == 0:
            hs = torch.empty((T,) + tuple(h0s.shape[1:]), dtype=torch.bfloat16, device=dev)
        _fused_forward_wide(wide, xs, h0s, hs, wA, wB, b32, B, T, N, F, G, K, H if direct else None, last_only, X if inline else None, st, gi=gi, gf=gf, scratch=scr)
        if not direct:
            _unpack_states(hs, H, last_only, N, st)
        if return_states:
            return hs_all, plan, H
        return H
    if hs.shape[0] == 0:                                 # (lean, and not the wide kernel after all: the step kernels keep the state image)
        hs = torch.empty((T,) + tuple(h0s.shape[1:]), dtype=torch.bfloat16, device=dev)
    wpack = _fused_pack_weights(wA, wB, st)
    if native_out:
        assert not return_states
        _fused_forward_steps(graph, xs, h0s, hs, wpack, b32, B, T, N, F, G, K, None, False, X if inline else None, st, gi, gf, evs)
        Hv = hs.permute(1, 0, 3, 2)[:, :, :, :N]                     # B x T x F x N, strides of the sequence-major image
        return Hv[:, T - 1:] if last_only else Hv
    H = torch.empty((B, 1 if last_only else T, F, N), dtype=torch.bfloat16, device=dev)
    _fused_forward_steps(graph, xs, h0s, hs, wpack, b32, B, T, N, F, G, K, H if direct else None, last_only, X if inline else None, st, gi, gf, evs)
    if not direct:
        _unpack_states(hs, H, last_only, N, st)
    if return_states:
        return hs_all, plan, H
    return H


def fused_cell_forward_native(xs, h0s, wA, wB, bias, graph, N):
    """Un-gated GGCRNNCell forward on sequence-major arrays end to end: xs [T][B][NPad][G] bf16 (rows >= N zero; G = 32 or 64: the
    fused kernels' input widths), h0s [B][NPad][F] bf16 or None (= zeros, every call site of the reference: train_rnn.py:256) ->
    hs [T][B][NPad][F] bf16 (rows >= N zero). No pack, no inline pack, no user-layout copy: the launch moves the algorithm's own
    bytes (read x_t, read h_{t-1}, write h_t). `hs.permute(1, 0, 3, 2)[..., :N]` is the reference's B x T x F x N view of it."""
    require_device(xs, wA, wB, bias)
    T, B, npad, G = xs.shape
    F = wA.shape[0]
    K = max(wA.shape[2], wB.shape[2])
    plan = graph.fused_plan()
    assert npad == plan['npad'] and xs.dtype == torch.bfloat16 and xs.is_contiguous() and wA.shape[3] == G
    st = _stream()
    hs_all = torch.empty((T + 1, B, npad, F), dtype=torch.bfloat16, device=xs.device)
    if h0s is None:
        hs_all[0].zero_()
    else:
        assert tuple(h0s.shape) == (B, npad, F) and h0s.dtype == torch.bfloat16
        hs_all[0].copy_(h0s)
    wpack = _fused_pack_weights(wA.detach(), wB.detach(), st)
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    wide = fused_wide_plan(graph, B, T, N, F, G, K, False)
    if wide is not None:
        _fused_forward_wide(wide, xs, hs_all[:1], hs_all[1:], wA, wB, b32, B, T, N, F, G, K, None, False, None, st)
        return hs_all[1:]
    _fused_forward_steps(graph, xs, hs_all[:1], hs_all[1:], wpack, b32, B, T, N, F, G, K, None, False, None, st)
    return hs_all[1:]


def to_sequence_major(X, graph):
    """user layout X [B][T][C][N] bf16 -> the fused kernels' sequence-major array [T][B][NPad][C] (rows >= N zero)."""
    require_device(X)
    B, T, Cc, N = X.shape
    npad = graph.fused_plan()['npad']
    Xc = X.contiguous()
    xs = torch.empty((T, B, npad, Cc), dtype=torch.bfloat16, device=X.device)
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(Xc), _p(xs), B, T, Cc, N, npad, None, _stream()), 'pack_seq')
    return xs


# ------------------------------------------------------------------------------------------ node-gated cell on the fused path
def fused_filter_output(xs, w, bias, graph, K, N, adjoint=False):
    """(w(S) x_t + bias) for every (t, b) in one launch: [T][B][NPad][F] bf16 sequence-major (gcrnn_fused_filter_output_bf16).
    xs [T][B][NPad][C] bf16; w F x 1 x k x C (k <= K taps); C == F runs the operand as a state, otherwise as [0 | x_t].
    adjoint: the shifts run on the adjoint graph (S^T): with transposed taps this is the filter's input gradient."""
    T, B, npad, Cin = xs.shape
    F = w.shape[0]
    plan = graph.fused_plan(adjoint=adjoint)
    plan16 = _adjoint_plan16(graph) if adjoint else _forward_plan16(graph)
    st = _stream()
    b32 = _bias_f32(bias, st)
    out = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=xs.device)
    if Cin == F:
        wp = _cached_pack('statetaps_f', (w.detach(),), int(K), st, lambda: _fused_pack_state_taps(w, K, st))
        check(lib.gcrnn_fused_filter_output_bf16(_p(xs), None, _p(wp), _p(b32), _p(out), *_fused_graph_args(plan16 or plan), B, T, N, F, 0, K,
                                                 plan.get('uniform_w', 0.0), 1 if plan16 else 0, st),
              'fused_filter_output')
    else:
        def pack_x():
            wd = _pad_tap_count(w.detach(), K)
            return _fused_pack_weights(wd, wd.new_zeros((F, 1, K, F)), st), torch.zeros((1, npad, F), dtype=torch.bfloat16, device=xs.device)
        wp, zero_h = _cached_pack('filtertaps_x', (w.detach(),), (int(K), int(npad)), st, pack_x)
        check(lib.gcrnn_fused_filter_output_bf16(_p(zero_h), _p(xs), _p(wp), _p(b32), _p(out), *_fused_graph_args(plan16 or plan), B, T, N, F, Cin, K,
                                                 plan.get('uniform_w', 0.0), 1 if plan16 else 0, st),
              'fused_filter_output')
    return out


def node_gate_logits(cs, wf, bf, graph, N):
    """GraphFilter_{F -> 1} of the gate-cell states (graphML.py:2387), taps first: s_k = cs . w_k per node (one pass over cs), then
    K-1 accumulate-SpMM hops on the ONE-channel signals in node-major layout [N][items]. cs [T][B][NPad][F] bf16, wf 1 x 1 x K x F,
    bf 1 x 1 or None -> logits [T][B][N] fp32 (and the pieces the backward needs)."""
    T, B, npad, F = cs.shape
    K = wf.shape[2]
    items = T * B
    wk = wf.detach().float().reshape(K, F).contiguous()
    s = torch.empty((items, K, 1, N), dtype=torch.float32, device=cs.device)
    for i0 in range(0, items, 32768):            # gridDim.y limit of the dot kernel
        n_i = min(32768, items - i0)
        check(lib.gcrnn_node_gate_dot(_p(cs.view(items, npad, F)[i0:]), _p(wk), _p(s[i0:]), n_i, N, npad, F, K, _stream()), 'node_gate_dot')
    return _node_gate_logits_from_taps(s, bf, graph, T, B, N), wk


def _node_gate_logits_from_taps(s, bf, graph, T, B, N):
    """Second stage of the F -> 1 GraphFilter: s [items][K][1][N] fp32 per-tap dot products -> logits [T][B][N] (K-1 Horner hops on
    the one-channel signals, node-major). s [items][S][K][1][N]: per-slice partials, added by the layout pass (gcrnn_pack_node_major_sum_f32)."""
    if s.dim() == 5:
        items, S_, K = s.shape[0], s.shape[1], s.shape[2]
        sn = torch.empty((K, N, items, 1), dtype=torch.float32, device=s.device)
        check(lib.gcrnn_pack_node_major_sum_f32(_p(s), _p(sn), items, S_, K, 1, N, _stream()), 'pack_node_major_sum')
    else:
        K = s.shape[1]
        sn = _pack_raw(s)                                              # [K][N][items][1]
    acc = sn[K - 1:K]
    csr = graph.fwd[0]
    for k in range(K - 2, -1, -1):
        spmm_raw(csr, acc, out=sn[k:k + 1], accumulate=True)         # sn[k] += P acc  (Horner)
        acc = sn[k:k + 1]
    logit = _unpack_raw(acc).view(T, B, N)                             # [items][1][1][N]
    if bf is not None:
        logit = logit + bf.detach().float().view(())
    return logit


def _tap_fragments(wf, F):
    """The F -> 1 filter's taps wf 1 x 1 x K x F (fp32) as the A fragments gcrnn_fused_gate_prepass_taps_bf16 takes: three bf16 planes
    (p0 + p1 + p2 = w to 24 bits), bf16 [F/16][3][64][4] with lane l = 16 kg + tap holding w_p[tap][16 chunk + 4 kg + e]."""
    K = wf.shape[2]
    w = wf.detach().float().reshape(K, F)
    p0 = w.to(torch.bfloat16)
    r1 = w - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    pl = torch.zeros((3, 16, F), dtype=torch.bfloat16, device=w.device)
    pl[:, :K] = torch.stack([p0, p1, p2])
    # [plane][tap][chunk][kg][e] -> [chunk][plane][kg][tap][e]
    return pl.view(3, 16, F // 16, 4, 4).permute(2, 0, 3, 1, 4).contiguous()


def fused_node_gate_taps(xs, h0s, wA_g, wB_g, bias_g, wf, graph, N, hzero=None, pending=None):
    """Gate cell of a node gate at inference with the per-tap dot products of its F -> 1 filter fused into the pre-pass
    (gcrnn_fused_gate_prepass_taps_bf16): returns s [T*B][K][1][N] fp32, or None where the fused pre-pass does not apply (the caller
    then stores the states and runs gcrnn_node_gate_dot over them). Lays out X too when xs still waits for its layout (pending: its _PendingLayout)."""
    T, B, npad, G = xs.shape
    F = wA_g.shape[0]
    K = max(wA_g.shape[2], wB_g.shape[2])
    Kt = wf.shape[2]
    plan = graph.fused_plan()
    plan16 = fused_img16_plan(graph, True, None)
    x_user = pending.settle(_gate_prepass_lays_out(plan, plan16, B, T, N, F, G, K)) if pending is not None else None
    if plan16 is None or os.environ.get('GCRNN_NO_FUSED_TAPS') or not int(lib.gcrnn_fused_gate_prepass_taps_supported(
            B, T, N, F, G, K, plan16['entries'], plan.get('uniform_w', 0.0), 1, 1 if x_user is not None else 0, Kt)):
        if x_user is not None:
            pending.x_user = x_user      # not laid out here after all: still pending, for the pre-pass the caller runs instead
        return None
    st = _stream()
    wp = _fused_pack_weights(wA_g.detach(), wB_g.detach(), st)
    bg = _bias_f32(bias_g, st)
    frags = _cached_pack('tapfrags', (wf.detach(),), int(F), st, lambda: _tap_fragments(wf, F))      # (parameter-derived: kept while wf is unchanged)
    s = torch.empty((T * B, Kt, 1, N), dtype=torch.float32, device=xs.device)
    check(lib.gcrnn_fused_gate_prepass_taps_bf16(_p(x_user), _p(xs), _p(h0s), _p(wp), _p(bg), _p(frags), _p(s), Kt, None,
                                                 *_fused_graph_args(plan16), B, T, N, F, G, K, _p(hzero), plan.get('uniform_w', 0.0), 1, st),
          'gate_prepass_taps')
    return s


def _tap_fragments32(wfs, F):
    """The F -> 1 filters' taps of BOTH node gates (each 1 x 1 x K x F) as the A fragments gcrnn_fused_gate_pair_prepass_taps_wide_bf16 takes:
    three bf16 planes (p0 + p1 + p2 = w to 24 bits), bf16 [2][F/32][3][64][8] with lane l = 16 kg + tap holding w_p[tap][32 cg + 8 kg .. + 7]."""
    out = []
    for wf in wfs:
        K = wf.shape[2]
        w = wf.detach().float().reshape(K, F)
        p0 = w.to(torch.bfloat16)
        r1 = w - p0.float()
        p1 = r1.to(torch.bfloat16)
        p2 = (r1 - p1.float()).to(torch.bfloat16)
        pl = torch.zeros((3, 16, F), dtype=torch.bfloat16, device=w.device)
        pl[:, :K] = torch.stack([p0, p1, p2])
        # [plane][tap][cg][kg][j] -> [cg][plane][kg][tap][j]
        out.append(pl.view(3, 16, F // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous())
    return torch.stack(out, dim=0).contiguous()


def fused_node_gate_taps_pair(xs, h0s, gate_in, gate_f, graph, N, hzero=None, pending=None):
    """BOTH node gates' cells of every (t, b) with the per-tap dot products of their F -> 1 filters, as ONE pre-pass launch of the wide
    sequence-resident kernel (gcrnn_fused_gate_pair_prepass_taps_wide_bf16; inference). gate_* = (wA_g, wB_g, bias_g, wf, bf) as in
    fused_node_cell_forward. Returns (s_in, s_f), each [T*B][K][1][N] fp32, or None where the wide pre-pass does not apply."""
    T, B, npad, G = xs.shape
    F = gate_in[0].shape[0]
    K = max(gate_in[0].shape[2], gate_in[1].shape[2])
    Kt = gate_in[3].shape[2]
    if gate_f[3].shape[2] != Kt or max(gate_f[0].shape[2], gate_f[1].shape[2]) != K or os.environ.get('GCRNN_NO_NODE_GATE_PAIR'):
        return None
    if fused_gate_pair_plan(graph, B, T, N, F, G, K, pending is not None and not pending.settled)[0] is None:
        return None
    x_user = pending.settle(fused_gate_pair_plan(graph, B, T, N, F, G, K, True)[1]) if pending is not None else None
    plan16, _ = fused_gate_pair_plan(graph, B, T, N, F, G, K, x_user is not None)
    if plan16 is None:
        return None
    st = _stream()

    def prepare():
        wA2 = torch.cat([_pad_gate_inputs(gate_in[0].detach(), G), _pad_gate_inputs(gate_f[0].detach(), G)], dim=0)
        wB2 = torch.cat([gate_in[1].detach(), gate_f[1].detach()], dim=0)
        wp_ = _fused_pack_weights_wide(wA2, wB2, plan16['uniform_w'], st)
        zb = torch.zeros(F, dtype=torch.float32, device=xs.device)
        b2_ = torch.cat([(g[2].detach().float().reshape(-1) if g[2] is not None else zb) for g in (gate_in, gate_f)]).contiguous()
        return wp_, b2_, _tap_fragments32((gate_in[3], gate_f[3]), F)
    ptens = tuple(t.detach() for g in (gate_in, gate_f) for t in g[:4] if t is not None)
    wp, b2, frags = _cached_pack('nodegatepair', ptens, (float(plan16['uniform_w']), tuple(t is None for g in (gate_in, gate_f) for t in g[:4])), st, prepare)
    nch = F // 32
    parts = torch.empty((T * B, 2, nch, Kt, N), dtype=torch.float32, device=xs.device)
    check(lib.gcrnn_fused_gate_pair_prepass_taps_wide_bf16(_p(x_user), _p(xs), _p(h0s), _p(wp), _p(b2), _p(frags), _p(parts), Kt, None, None,
                                                           *_wide_graph_args(plan16), B, T, N, F, G, K, _p(hzero), _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st),
          'gate_pair_prepass_taps')
    return parts.view(T * B * 2, nch, Kt, 1, N)                         # row 2 i + g: item i, gate g; [.., chunk, tap, 1, node]: the caller's layout pass adds the chunks


def fused_node_supported(graph, N, F, G, Kin, Kst, dtype, E=1):
    """Node-gated cell on the fused kernels: the fused shapes in bf16 plus a state-only instantiation for K = max(Kin, Kst)."""
    return fused_supported(N, F, G, Kin, Kst, dtype, E) and max(Kin, Kst) in (2, 3, 4, 5) and not (max(Kin, Kst) == 4 and F == 32)


def fused_node_cell_forward(X, h0, wA, wB, bias, graph, node_gates, time_gates=None, last_only=False):
    """Node-gated GGCRNNCell forward (optionally time-gated too) on the fused kernels (graphML.py:2379-2407, 2420-2423).
    node_gates = {'in': (wA_g, wB_g, bias_g, wf, bf), 'forget': (...)}: the gate cell GRNN_node_* and its F -> 1 GraphFilter
    GFL_node_*; time_gates as in fused_cell_forward. X B x T x G x N bf16, h0 B x F x N bf16 -> H B x T x F x N bf16.
    Everything that does not depend on h_{t-1} -- both gate cells, their filters, A(S)x_t + b -- runs for all T steps at once.
    Inference (no autograd graph is recorded here; training goes through fused_node_cell_train)."""
    require_device(X, h0, wA, wB, bias)
    X, wA = fused_pad_operands(X, wA.detach())
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan()
    st = _stream()
    xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0.contiguous(), graph, F, K)      # (the first gate cell's pre-pass lays out the rest of X)
    h0s, hs = hs_all[:1], hs_all[1:]
    hzero = fused_h0_zero_flag(h0)
    zero_lin = torch.zeros((1, F * N), dtype=torch.float32, device=X.device)
    ng = []
    pair = fused_node_gate_taps_pair(xs, h0s, node_gates['in'], node_gates['forget'], graph, N, hzero=hzero, pending=pending)      # both gate cells in ONE launch (wide kernel)
    ngates = None
    if pair is not None and not os.environ.get('GCRNN_NO_NODE_GATE_FILTER') and int(lib.gcrnn_node_gate_filter_supported(pair.shape[2], N, graph.fwd[0].nnz, plan.get('uniform_w', 0.0))):
        # second stage of both F -> 1 filters in ONE pass over the tap dots: chunk sum, the K - 1 one-channel hops (running signal in LDS),
        # each gate's bias, the sigmoid, written as the recurrence reads them (gcrnn_node_gate_filter_f32)
        bfs = tuple(node_gates[name][4] for name in ('in', 'forget'))
        b2 = None
        if any(b is not None for b in bfs):
            b2 = _cached_pack('nodegatebias', tuple(b.detach() for b in bfs if b is not None), tuple(b is None for b in bfs), st,
                              lambda: torch.cat([(b.detach().float().reshape(1) if b is not None else torch.zeros(1, device=X.device)) for b in bfs]).contiguous())
        csr = graph.fwd[0]
        ngates = torch.empty((T, 2, B, N), dtype=torch.float32, device=X.device)
        check(lib.gcrnn_node_gate_filter_f32(_p(pair), _p(ngates), T * B * 2, pair.shape[1], pair.shape[2], N, 2, B, _p(csr.rowptr), _p(csr.col),
                                             _p(csr.val(torch.float32)), csr.nnz, plan.get('uniform_w', 0.0), _p(b2), 1, st), 'node_gate_filter')
    elif pair is not None:
        lg = _node_gate_logits_from_taps(pair, None, graph, T, B * 2, N).view(T, B, 2, N)
        for gidx, name in enumerate(('in', 'forget')):
            bf = node_gates[name][4]
            l1 = lg[:, :, gidx]
            ng.append(torch.sigmoid(l1 + bf.detach().float().view(()) if bf is not None else l1))
    for name in (() if pair is not None else ('in', 'forget')):
        wA_g, wB_g, bias_g, wf, bf = node_gates[name]
        wA_g = _pad_gate_inputs(wA_g, G)
        staps = fused_node_gate_taps(xs, h0s, wA_g, wB_g, bias_g, wf, graph, N, hzero=hzero, pending=pending)
        if staps is not None:          # the filter's tap dots came out of the pre-pass itself: no state array, no pass over it
            logit = _node_gate_logits_from_taps(staps, bf, graph, T, B, N)
        else:
            _, cs, _ = fused_time_gate(xs, h0s, wA_g, wB_g, bias_g, zero_lin, None, graph, N, store_states=True, hzero=hzero, pending=pending)
            logit, _ = node_gate_logits(cs, wf, bf, graph, N)
        ng.append(torch.sigmoid(logit))
    if ngates is None:
        ngates = torch.stack(ng, dim=1).contiguous()                    # [T][2][B][N]
    assert pending is None or pending.settled
    gi = gf = None
    if time_gates is not None:
        gi, gf = _fused_time_gates_each(xs, h0s, time_gates, graph, N, hzero)
    plan16 = fused_img16_plan(graph, False, None)
    uw = float(plan.get('uniform_w', 0.0))
    b32 = _bias_f32(bias, st)
    # (round 5) both state-size passes on the WIDE kernel when it takes them: A(S) x_t + b over all items (mode 3) and the recurrence with the
    # per-node gates in its epilogue as ONE launch (mode 4); else round 3's 16-feature kernels
    if plan16 is not None and F % 32 == 0 and G % 32 == 0 and lib.gcrnn_fused_filter_output_wide_supported(B, T, N, F, G, K, int(plan16['entries']), uw, 1, 0):
        wpx = _fused_pack_weights_wide(wA.detach(), wA.new_zeros((F, 1, K, F)), uw, st)      # (zero state taps, K of them: the pack's tap count is the kernel's)
        yx = torch.empty((T, B, plan['npad'], F), dtype=torch.bfloat16, device=X.device)
        check(lib.gcrnn_fused_filter_output_wide_bf16(_p(xs), _p(wpx), _p(b32), _p(yx), *_wide_graph_args(plan16), B, T, N, F, G, K, None, st),
              'fused_filter_output_wide')
    else:
        yx = fused_filter_output(xs, wA, bias, graph, K, N)
    H = torch.empty((B, 1 if last_only else T, F, N), dtype=torch.bfloat16, device=X.device)
    direct = (N % 8 == 0)
    if plan16 is not None and F % 32 == 0 and lib.gcrnn_fused_node_forward_wide_supported(B, T, N, F, K, int(plan16['entries']), uw, 1):
        wBk = _pad_tap_count(wB.detach(), K)
        wpBw = _fused_pack_weights_wide(wB.new_zeros((F, 1, 1, 0)), wBk, uw, st)      # (state-only operand: G = 0)
        check(lib.gcrnn_fused_node_forward_wide_bf16(_p(h0s), _p(hs), _p(yx), _p(ngates), _p(gi), _p(gf), _p(wpBw), _p(b32),
                                                     *_wide_graph_args(plan16), B, T, N, F, K,
                                                     _p(H) if direct else None, int(last_only), st), 'fused_node_forward_wide')
        if not direct:
            _unpack_states(hs, H, last_only, N, st)
        return H
    def pack_state():
        wBk = _pad_tap_count(wB.detach(), K)
        return _fused_pack_state_taps(wBk, K, st)
    wpB = _cached_pack('statetaps', (wB.detach(),), int(K), st, pack_state)
    check(lib.gcrnn_fused_node_forward_bf16(_p(h0s), _p(hs), _p(yx), _p(ngates), _p(gi), _p(gf), _p(wpB), _p(b32), None,
                                            *_fused_graph_args(plan16 or plan), B, T, N, F, K, _p(H) if direct else None,
                                            int(last_only) | (2 if plan16 else 0), plan.get('uniform_w', 0.0), st),
          'fused_node_forward')
    if not direct:
        _unpack_states(hs, H, last_only, N, st)
    return H


class _FusedNodeGate(torch.autograd.Function):
    """One node gate of the fused path with its BPTT (graphML.py:2379-2399): gate[t][b][n] = sigmoid(GraphFilter_{F->1}(c_t))[n],
    c_t = tanh(A_g(S)x_t + B_g(S)h0 + 2 b_g) the state of the gate cell GRNN_node_*.
    forward  = the gate pre-pass over all (t, b) storing c, the taps-first F -> 1 filter (node_gate_logits), sigmoid;
    backward = adjoint Horner of the one-channel hops, one pass over c (filter-weight gradient + the gate cell's pre-activation
               gradient in place), then the weight-gradient kernel with h0 as every item's state operand. No gradient for X / h0."""

    @staticmethod
    def forward(ctx, xs, h0s, X, h0, wA_g, wB_g, bias_g, wf, bf, graph, hzero, pending=None):
        N, F = X.shape[3], wA_g.shape[0]
        zero_lin = torch.zeros((1, F * N), dtype=torch.float32, device=X.device)
        _, cs, _ = fused_time_gate(xs, h0s, wA_g, wB_g, bias_g, zero_lin, None, graph, N, store_states=True, hzero=hzero, pending=pending)
        logit, wk = node_gate_logits(cs, wf, bf, graph, N)
        gate = torch.sigmoid(logit)
        ctx.save_for_backward(X, h0, wA_g, wB_g, bias_g, wf, bf, gate, cs, wk, hzero)
        ctx.graph = graph
        return gate

    @staticmethod
    def backward(ctx, dgate):
        X, h0, wA_g, wB_g, bias_g, wf, bf, gate, cs, wk, hzero = ctx.saved_tensors
        if getattr(ctx, 'consumed', False):
            raise GcrnnError('the fused node gate was already back-propagated (its saved states are turned into gradients in place)')
        ctx.consumed = True
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            raise GcrnnError('the fused node gate does not produce gradients w.r.t. X or h0')
        graph = ctx.graph
        B, T, G, N = X.shape
        F, Kin, Kst = wA_g.shape[0], wA_g.shape[2], wB_g.shape[2]
        Kc = max(Kin, Kst)
        K = wf.shape[2]
        npad = cs.shape[2]
        items = T * B
        dlogit = (dgate.float() * gate * (1.0 - gate)).contiguous()                     # through the sigmoid: [T][B][N]
        # logit = sum_k P^k s_k + b  =>  d s_k = (P^T)^k dlogit: K-1 one-channel hops with the adjoint graph (CSR(S))
        dn = torch.empty((K, N, items, 1), dtype=torch.float32, device=X.device)
        dn[0:1] = _pack_raw(dlogit.view(items, 1, 1, N))
        for k in range(1, K):
            spmm_raw(graph.adj[0], dn[k - 1:k], out=dn[k:k + 1])
        ds = _unpack_raw(dn)                                                              # [items][K][1][N]
        dw_part = torch.empty((items, K, F), dtype=torch.float32, device=X.device)
        check(lib.gcrnn_node_gate_dot_backward(_p(cs), _p(ds), _p(wk), _p(dw_part), items, N, npad, F, K, _stream()), 'node_gate_dot_backward')
        gwf = dw_part.sum(dim=0).view(1, 1, K, F).to(wf.dtype) if ctx.needs_input_grad[7] else None
        gbf = dlogit.sum().view_as(bf).to(bf.dtype) if (bf is not None and ctx.needs_input_grad[8]) else None
        # cs now holds the gate cell's pre-activation gradient
        dW, dbs = fused_backward_weight(cs, X, None, h0, graph, F, G, Kc, want_bias=True, h_is_h0=True, hzero=hzero)
        gA = dW[:, :Kin, F:].unsqueeze(1).to(wA_g.dtype) if ctx.needs_input_grad[4] else None
        gB = dW[:, :Kst, :F].unsqueeze(1).to(wB_g.dtype) if ctx.needs_input_grad[5] else None
        gb = dbs.view_as(bias_g).to(bias_g.dtype) if (bias_g is not None and ctx.needs_input_grad[6]) else None
        return None, None, None, None, gA, gB, gb, gwf, gbf, None, None, None


class _FusedNodeCell(torch.autograd.Function):
    """Node-gated GGCRNNCell (optionally time-gated too) on the fused kernels with its BPTT; the gates enter as differentiable
    inputs ni, nf [T][B][N] (and gi, gf [T][B] or None). backward = data chain with the per-node forget gates folded into every
    launch's operand -> one all-items pass for the gate gradients and the x filter's pre-activation gradient -> two weight-gradient
    launches (input filter on gi ni . dpre, state filter on gf nf . dpre). No gradient for X or h0."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, ni, nf, gi, gf, graph, xs, hs_all):
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        plan = graph.fused_plan()
        st = _stream()
        h0s, hs = hs_all[:1], hs_all[1:]
        yx = fused_filter_output(xs, wA, bias, graph, K, N)
        ngates = torch.stack([ni.detach().float(), nf.detach().float()], dim=1).contiguous()
        gic = gi.detach().float().contiguous() if gi is not None else None
        gfc = gf.detach().float().contiguous() if gf is not None else None
        wBk = _pad_tap_count(wB.detach(), K)
        wpB = _fused_pack_state_taps(wBk, K, st)
        b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
        H = torch.empty((B, T, F, N), dtype=torch.bfloat16, device=X.device)
        yh = torch.empty_like(yx)
        plan16 = fused_img16_plan(graph, False, None)
        check(lib.gcrnn_fused_node_forward_bf16(_p(h0s), _p(hs), _p(yx), _p(ngates), _p(gic), _p(gfc), _p(wpB), _p(b32), _p(yh),
                                                *_fused_graph_args(plan16 or plan), B, T, N, F, K, _p(H), 2 if plan16 else 0,
                                                plan.get('uniform_w', 0.0), st), 'fused_node_forward')
        ctx.save_for_backward(X, h0, wA, wB, bias, H, hs_all, yx, yh, ngates, gic, gfc)
        ctx.graph, ctx.npad = graph, plan['npad']
        return H

    @staticmethod
    def backward(ctx, dH):
        X, h0, wA, wB, bias, H, hs_all, yx, yh, ngates, gi, gf = ctx.saved_tensors
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise GcrnnError('the fused node-gated BPTT does not produce gradients w.r.t. X or h0')
        graph, npad = ctx.graph, ctx.npad
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        st = _stream()
        hs = hs_all[1:]
        dH = dH.to(torch.bfloat16).contiguous()
        dHs, dHu = fused_pack_upstream(dH, graph, K)
        ngf = (ngates[:, 1] * gf.unsqueeze(2)).contiguous() if gf is not None else ngates[:, 1].contiguous()       # [T][B][N]
        wBk = _pad_tap_count(wB.detach(), K)
        wBt = _transposed_taps(wBk)                                                     # [F_in][1][K][F_out]
        wpT = _fused_pack_state_taps(wBt, K, st)
        aplan = graph.fused_plan(adjoint=True)
        aplan16 = _adjoint_plan16(graph)
        dpre = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=X.device)
        dyh = torch.empty_like(dpre)
        check(lib.gcrnn_fused_node_backward_data_bf16(_p(dHs), _p(hs), _p(dpre), _p(dyh), _p(ngf), _p(wpT), *_fused_graph_args(aplan16 or aplan),
                                                      B, T, N, F, K, aplan.get('uniform_w', 0.0), _p(dHu), 1 if aplan16 else 0, st), 'fused_node_backward_data')
        dyx = torch.empty_like(dpre)
        dni = torch.empty((T, B, N), dtype=torch.float32, device=X.device)
        dnf = torch.empty_like(dni)
        dgi = torch.empty((T, B), dtype=torch.float32, device=X.device) if gi is not None else None
        dgf = torch.empty((T, B), dtype=torch.float32, device=X.device) if gf is not None else None
        check(lib.gcrnn_node_cell_backward(_p(dpre), _p(yx), _p(yh), _p(ngates), _p(gi), _p(gf), _p(dyx), _p(dni), _p(dnf), _p(dgi), _p(dgf),
                                           B, T, N, npad, F, st), 'node_cell_backward')
        one = torch.ones((T, B), dtype=torch.float32, device=X.device)
        zero = torch.zeros_like(one)
        dWx, dbx = fused_backward_weight(dyx, X, H, h0, graph, F, G, K, want_bias=True, gi=one, gf=zero)      # input-filter columns
        dWh, dbh = fused_backward_weight(dyh, X, H, h0, graph, F, G, K, want_bias=True, gi=zero, gf=one)      # state-filter columns
        gA = dWx[:, :Kin, F:].unsqueeze(1).to(wA.dtype) if ctx.needs_input_grad[2] else None
        gB = dWh[:, :Kst, :F].unsqueeze(1).to(wB.dtype) if ctx.needs_input_grad[3] else None
        gb = (dbx + dbh).view_as(bias).to(bias.dtype) if (bias is not None and ctx.needs_input_grad[4]) else None
        return (None, None, gA, gB, gb, dni if ctx.needs_input_grad[5] else None, dnf if ctx.needs_input_grad[6] else None,
                dgi if (gi is not None and ctx.needs_input_grad[7]) else None, dgf if (gf is not None and ctx.needs_input_grad[8]) else None,
                None, None, None)


def fused_node_cell_train(X, h0, wA, wB, bias, graph, node_gates, time_gates=None):
    """Training forward of the node-gated (optionally time + node gated) cell on the fused kernels: every gate sub-network is an
    autograd node of its own (_FusedNodeGate / _FusedTimeGate) and enters the cell (_FusedNodeCell) as a differentiable input."""
    require_device(X, h0, wA, wB, bias)
    with torch.no_grad():
        xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0, graph, wA.shape[0], max(wA.shape[2], wB.shape[2]))
        hzero = fused_h0_zero_flag(h0)
    ni = _FusedNodeGate.apply(xs, hs_all[:1], X, h0, *node_gates['in'], graph, hzero, pending)
    nf = _FusedNodeGate.apply(xs, hs_all[:1], X, h0, *node_gates['forget'], graph, hzero)
    assert pending is None or pending.settled                   # (the first pre-pass laid out the rest of X)
    gi = gf = None
    if time_gates is not None:
        gi, gf = fused_train_time_gates(xs, hs_all[:1], X, h0, time_gates, graph, hzero)
    return _FusedNodeCell.apply(X, h0, wA, wB, bias, ni, nf, gi, gf, graph, xs, hs_all)


# ------------------------------------------------------------------------------------------ edge-gated cell, fused path
def fused_edge_supported(graph, N, F, G, Kin, Kst, dtype, E=1):
    """Edge-gated cell on the fused kernels: the node-gated path's shapes (state-only instantiation of the step kernel for the
    filter passes) plus the attention kernel's (N % 8 == 0, z [N][F] bf16 and the per-node scalars in LDS)."""
    return fused_node_supported(graph, N, F, G, Kin, Kst, dtype, E) and bool(lib.gcrnn_fused_edge_attention_supported(int(N), int(F)))


def _edge_composite(w, bias, att_w):
    """The attention's mixing matrix folded into a filter: z = W (sum_k S^k u C_k + b) = sum_k S^k u (W C_k) + W b
    (W acts on features, S on nodes). w F x 1 x k x C, bias F x 1 or None, att_w 1 x 1 x F x F -> (W C) F x 1 x k x C fp32, W b [F]."""
    W = att_w[0, 0].float()
    wc = torch.einsum('pf,fekc->pekc', W, w.float())
    bc = (W @ bias.float().view(-1)) if bias is not None else None
    return wc, bc


def fused_edge_attention(z, a12, graph, gx=None, gi=None, gf=None, out=None, r_out=None, Huser=None, huser_item_stride=0, N=None,
                         negative_slope=0.2):
    """The attention of the fused edge gate (gcrnn_fused_edge_attention_bf16) on the items of z [..][NPad][F] bf16 (leading dims =
    items). gx None: relu(att(z)); else tanh(gi gx + gf relu(att(z))) with per-item scalars gi / gf (fp32, or None)."""
    npad, F = z.shape[-2], z.shape[-1]
    items = z.numel() // (npad * F)
    ep = graph.edge_plan()
    if out is None:
        out = torch.empty_like(z)
    check(lib.gcrnn_fused_edge_attention_bf16(_p(z), _p(a12), _p(gx), _p(gi), _p(gf), _p(ep['rowptr']), _p(ep['r_edge']),
                                              _p(ep['t_rowptr']), _p(ep['t_edge']), _p(ep['t_order']), _p(out), _p(r_out), _p(Huser), int(huser_item_stride),
                                              items, int(N if N is not None else graph.N), npad, F, float(negative_slope), _stream()),
          'fused_edge_attention')
    return out


def fused_edge_cell_forward(X, h0, wA, wB, bias, graph, att_in, att_f, time_gates=None, last_only=False, negative_slope=0.2):
    """Edge-gated GGCRNNCell forward (optionally time-gated too) on the fused kernels (graphML.py:2409-2416, 2420-2423).
    att_in / att_f = (mixer 1 x 1 x 2F, weight 1 x 1 x F x F) of input_attention / forget_attention; time_gates as in
    fused_cell_forward. X B x T x G x N bf16, h0 B x F x N bf16 -> H B x T x F x N bf16 (B x 1 x F x N with last_only).
    The x branch relu(att_in(A(S)x_t + b)) does not depend on the recurrence: one filter pass and one attention pass over all
    T * B items; every step is then two launches: the state filter pass (composite taps) and the attention + tanh epilogue.
    Inference only (training goes through fused_edge_cell_train)."""
    require_device(X, h0, wA, wB, bias)
    X, wA = fused_pad_operands(X, wA.detach())
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan()
    npad = plan['npad']
    st = _stream()
    x_pending = None
    if time_gates is not None:      # (the first time-gate pre-pass lays out the rest of X)
        xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0.contiguous(), graph, F, K)
    else:
        # (round 5) without time gates the first consumer of xs is the x branch's filter pass: when the wide kernel takes it, only the leading
        # time step(s) are laid out here and its items lay out the rest while they run -- no separate pass over X (0.5 ms at B = 256, T = 32)
        Xc = X.contiguous()
        p16_ = fused_img16_plan(graph, True, None)
        steps = 0
        if (p16_ is not None and F % 32 == 0 and G % 32 == 0 and Xc.dtype == torch.bfloat16 and Xc.data_ptr() % 16 == 0
                and not os.environ.get('GCRNN_NO_INLINE_PACK')):
            steps = int(lib.gcrnn_fused_filter_output_wide_supported(B, T, N, F, G, K, int(p16_['entries']), float(plan.get('uniform_w', 0.0)), 1, 1))
        if 0 < steps < T:
            xs, hs_all = _pack_leading_steps(Xc, h0, npad, F, steps)
            x_pending = Xc
        else:
            xs, hs_all = fused_pack_inputs(Xc, h0.contiguous(), graph)
    gi = gf = None
    if time_gates is not None:
        hzero = fused_h0_zero_flag(h0)
        gi, gf = (g.contiguous() for g in _fused_time_gates_each(xs, hs_all[:1], time_gates, graph, N, hzero, pending))
        assert pending is None or pending.settled
    wAc, bA = _edge_composite(wA.detach(), bias.detach() if bias is not None else None, att_in[1].detach())
    wBc, bB = _edge_composite(wB.detach(), bias.detach() if bias is not None else None, att_f[1].detach())
    a_in = att_in[0].detach().float().reshape(2, F).contiguous()
    a_f = att_f[0].detach().float().reshape(2, F).contiguous()
    plan16 = fused_img16_plan(graph, False, None)
    uw = float(plan.get('uniform_w', 0.0))
    # (round 5) both filter passes on the WIDE kernel's filter-output mode when it takes them (csrc/gcrnn_fused_seq32.h mode 3: 32-feature chunks,
    # one workgroup per item): the x branch over all T B items, and per step the state filter with h_{t-1} as the mode's "input" operand
    wide_x = plan16 is not None and F % 32 == 0 and G % 32 == 0 and bool(lib.gcrnn_fused_filter_output_wide_supported(B, T, N, F, G, K, int(plan16['entries']), uw, 1, 0))
    wide_h = plan16 is not None and F % 32 == 0 and bool(lib.gcrnn_fused_filter_output_wide_supported(B, 1, N, F, F, K, int(plan16['entries']), uw, 1, 0))
    if wide_x:
        wpx = _fused_pack_weights_wide(wAc.contiguous(), wAc.new_zeros((F, 1, K, F)), uw, st)
        zx = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=X.device)
        check(lib.gcrnn_fused_filter_output_wide_bf16(_p(xs), _p(wpx), _p(bA.contiguous() if bA is not None else None), _p(zx),
                                                      *_wide_graph_args(plan16), B, T, N, F, G, K, _p(x_pending), st), 'fused_filter_output_wide')
    else:
        assert x_pending is None      # (the partial layout above was sized by the same query)
        zx = fused_filter_output(xs, wAc, bA, graph, K, N)                  # [T][B][NPad][F]
    gx = fused_edge_attention(zx, a_in, graph, out=zx, N=N, negative_slope=negative_slope)      # in place: every workgroup reads its item first
    wBc = _pad_tap_count(wBc, K)
    bB32 = bB.contiguous() if bB is not None else None
    if wide_h:
        wpBw = _fused_pack_weights_wide(wBc.contiguous(), wBc.new_zeros((F, 1, K, F)), uw, st)      # the state taps as the "input" taps of [0 | h_{t-1}]
    else:
        wpB = _fused_pack_state_taps(wBc, K, st)
    H = torch.empty((B, 1 if last_only else T, F, N), dtype=torch.bfloat16, device=X.device)
    zh = torch.empty((1, B, npad, F), dtype=torch.bfloat16, device=X.device)
    ga = _fused_graph_args(plan16 or plan)
    for t in range(T):
        if wide_h:
            check(lib.gcrnn_fused_filter_output_wide_bf16(_p(hs_all[t]), _p(wpBw), _p(bB32), _p(zh), *_wide_graph_args(plan16), B, 1, N, F, F, K, None, st), 'fused_filter_output_wide')
        else:
            check(lib.gcrnn_fused_filter_output_bf16(_p(hs_all[t]), None, _p(wpB), _p(bB32), _p(zh), *ga, B, 1, N, F, 0, K, uw, 1 if plan16 else 0, st),
                  'fused_filter_output')
        hu = None
        if not last_only:
            hu = H[:, t]
        elif t == T - 1:
            hu = H[:, 0]
        fused_edge_attention(zh, a_f, graph, gx=gx[t], gi=gi[t] if gi is not None else None, gf=gf[t] if gf is not None else None,
                             out=hs_all[t + 1], Huser=hu, huser_item_stride=(1 if last_only else T) * F * N, N=N,
                             negative_slope=negative_slope)
    return H


def fused_edge_training_supported(graph, N, F, G, Kin, Kst, E=1):
    """Edge-gated training on the fused kernels: the fused BPTT's shapes and the attention kernels' (hub rows beyond the backward
    kernel's 32 register-resident edge records take its slower chunked loop)."""
    if not (fused_training_supported(graph, N, F, G, Kin, Kst, E) and fused_edge_supported(graph, N, F, G, Kin, Kst, torch.bfloat16, E)):
        return False
    return bool(lib.gcrnn_fused_edge_attention_backward_supported(int(N), int(F), int(graph.edge_plan()['max_out_degree'])))


def fused_edge_attention_backward(dpre, r, g, z, a12, graph, N, scratch=None, negative_slope=0.2, dz=None, da_part=None, dgate=None):
    """Backward of fused_edge_attention for one branch over the items of dpre [..][NPad][F] (gcrnn_fused_edge_attention_backward_bf16):
    returns (dz like z, da_part fp32 [items][2][F], dgate fp32 [items] or None); dz / da_part / dgate: optional output buffers."""
    npad, F = z.shape[-2], z.shape[-1]
    items = z.numel() // (npad * F)
    ep = graph.edge_plan()
    if dz is None:
        dz = torch.empty_like(z)
    if da_part is None:
        da_part = torch.empty((items, 2, F), dtype=torch.float32, device=z.device)
    if dgate is None and g is not None:
        dgate = torch.empty((items,), dtype=torch.float32, device=z.device)
    if scratch is None:
        scratch = torch.empty((items, ep['nnz']), dtype=torch.float32, device=z.device)
    assert scratch.numel() >= items * ep['nnz']
    check(lib.gcrnn_fused_edge_attention_backward_bf16(_p(dpre), _p(r), _p(g), _p(z), _p(a12), _p(ep['rowptr']), _p(ep['r_edge']),
                                                       _p(ep['r_order']), _p(ep['t_rowptr']), _p(ep['t_pos']), _p(scratch), _p(dz),
                                                       _p(da_part), _p(dgate), items, int(N), npad, F, ep['nnz'], int(ep['max_out_degree']), float(negative_slope),
                                                       _stream()), 'fused_edge_attention_backward')
    return dz, da_part, dgate


class _FusedEdgeCell(torch.autograd.Function):
    """Edge-gated GGCRNNCell (optionally time-gated too) on the fused kernels with its BPTT (graphML.py:2409-2416 under autograd).
    forward: the x branch for all steps (filter pass with composite taps W_in A_k, attention), then two launches per step (state
    filter pass with W_f B_k, attention + tanh), keeping z, relu(att(z)) of both branches.
    backward, per step from the end: attention backward (dz_t, mixer partials, d gf_t) -> one launch of the data chain on dz_t
    (-> dpre_{t-1}); then the x branch's attention backward over all items, two weight-gradient launches (composite taps of the
    two filters) and the chain rule from the composite taps back to (taps, mixing matrix, bias). No gradient for X or h0."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, mix_in, w_in, mix_f, w_f, gi, gf, graph, xs, hs_all, slope):
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        plan = graph.fused_plan()
        npad = plan['npad']
        st = _stream()
        bd = bias.detach() if bias is not None else None
        wAc, bA = _edge_composite(wA.detach(), bd, w_in.detach())
        wBc, bB = _edge_composite(wB.detach(), bd, w_f.detach())
        a_in = mix_in.detach().float().reshape(2, F).contiguous()
        a_f = mix_f.detach().float().reshape(2, F).contiguous()
        gic = gi.detach().float().contiguous() if gi is not None else None
        gfc = gf.detach().float().contiguous() if gf is not None else None
        zx = fused_filter_output(xs, wAc, bA, graph, K, N)
        gx = fused_edge_attention(zx, a_in, graph, N=N, negative_slope=slope)
        wBk = _pad_tap_count(wBc, K)
        wpB = _fused_pack_state_taps(wBk, K, st)
        bB32 = bB.contiguous() if bB is not None else None
        H = torch.empty((B, T, F, N), dtype=torch.bfloat16, device=X.device)
        zh = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=X.device)
        rh = torch.empty_like(zh)
        plan16 = fused_img16_plan(graph, False, None)
        ga = _fused_graph_args(plan16 or plan)
        uw = plan.get('uniform_w', 0.0)
        for t in range(T):
            check(lib.gcrnn_fused_filter_output_bf16(_p(hs_all[t]), None, _p(wpB), _p(bB32), _p(zh[t]), *ga, B, 1, N, F, 0, K, uw, 1 if plan16 else 0, st),
                  'fused_filter_output')
            fused_edge_attention(zh[t], a_f, graph, gx=gx[t], gi=gic[t] if gic is not None else None,
                                 gf=gfc[t] if gfc is not None else None, out=hs_all[t + 1], r_out=rh[t], Huser=H[:, t],
                                 huser_item_stride=T * F * N, N=N, negative_slope=slope)
        ctx.save_for_backward(X, h0, wA, wB, bias, mix_in, w_in, mix_f, w_f, H, hs_all, zx, gx, zh, rh, gic, gfc, wBk)
        ctx.graph, ctx.npad, ctx.slope = graph, npad, slope
        return H

    @staticmethod
    def backward(ctx, dH):
        X, h0, wA, wB, bias, mix_in, w_in, mix_f, w_f, H, hs_all, zx, gx, zh, rh, gi, gf, wBk = ctx.saved_tensors
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise GcrnnError('the fused edge-gated BPTT does not produce gradients w.r.t. X or h0')
        graph, npad, slope = ctx.graph, ctx.npad, ctx.slope
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        st = _stream()
        dev = X.device
        hs = hs_all[1:]
        a_in = mix_in.detach().float().reshape(2, F).contiguous()
        a_f = mix_f.detach().float().reshape(2, F).contiguous()
        dH = dH.to(torch.bfloat16).contiguous()
        dHs, dHu = fused_pack_upstream(dH, graph, K)          # uniform graphs: only the last two steps; the chain launches lay out the rest
        wBt = _transposed_taps(wBk)                                                 # transposed composite taps [F_in][1][K][F_out]
        wpT = _fused_pack_state_taps(wBt, K, st)
        aplan = graph.fused_plan(adjoint=True)
        aplan16 = _adjoint_plan16(graph)
        aga = _fused_graph_args(aplan16 or aplan)
        auw = aplan.get('uniform_w', 0.0)
        nnz = graph.edge_plan()['nnz']
        tchunk = max(1, min(T, (1 << 26) // max(1, B * nnz)))                       # <= 256 MiB of per-edge scratch
        scratch = torch.empty((tchunk * B, nnz), dtype=torch.float32, device=dev)
        dpre = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=dev)
        dzh = torch.empty_like(dpre)
        da_f = torch.empty((T, B, 2, F), dtype=torch.float32, device=dev)
        dgf = torch.empty((T, B), dtype=torch.float32, device=dev) if gf is not None else None
        step = B * npad * F
        check(lib.gcrnn_fused_backward_seed_bf16(_p(dHs[T - 1]), _p(hs[T - 1]), _p(dpre[T - 1]), step, st), 'backward_seed')
        for t in range(T - 1, -1, -1):
            fused_edge_attention_backward(dpre[t], rh[t], gf[t] if gf is not None else None, zh[t], a_f, graph, N, scratch=scratch,
                                          negative_slope=slope, dz=dzh[t], da_part=da_f[t], dgate=dgf[t] if dgf is not None else None)
            if t > 0:
                nxt = dHu is not None and t >= 2
                check(lib.gcrnn_fused_backward_step_bf16(_p(dzh[t]), _p(dHs[t - 1]), _p(hs[t - 1]), _p(dpre[t - 1]), _p(wpT), *aga,
                                                         B, N, F, K, auw, _p(dHu[:, t - 2]) if nxt else None, _p(dHs[t - 2]) if nxt else None, T,
                                                         1 if aplan16 else 0, st),
                      'fused_backward_step')
        dzx = torch.empty_like(dpre)
        da_i = torch.empty((T, B, 2, F), dtype=torch.float32, device=dev)
        dgi = torch.empty((T, B), dtype=torch.float32, device=dev) if gi is not None else None
        for t0 in range(0, T, tchunk):
            t1 = min(T, t0 + tchunk)
            fused_edge_attention_backward(dpre[t0:t1], gx[t0:t1], gi[t0:t1] if gi is not None else None, zx[t0:t1], a_in, graph, N,
                                          scratch=scratch, negative_slope=slope, dz=dzx[t0:t1], da_part=da_i[t0:t1],
                                          dgate=dgi[t0:t1] if dgi is not None else None)
        one = torch.ones((T, B), dtype=torch.float32, device=dev)
        zero = torch.zeros_like(one)
        dWx, dbx = fused_backward_weight(dzx, X, H, h0, graph, F, G, K, want_bias=True, gi=one, gf=zero)       # composite input taps
        dWh, dbh = fused_backward_weight(dzh, X, H, h0, graph, F, G, K, want_bias=True, gi=zero, gf=one)       # composite state taps
        dAc, dBc = dWx[:, :Kin, F:], dWh[:, :Kst, :F]                                 # [F'][k][C] fp32
        Wi, Wf = w_in.detach()[0, 0].float(), w_f.detach()[0, 0].float()
        A32, B32 = wA.detach()[:, 0].float(), wB.detach()[:, 0].float()              # [F][k][C]
        gA = torch.einsum('pf,pkc->fkc', Wi, dAc).unsqueeze(1).to(wA.dtype) if ctx.needs_input_grad[2] else None
        gB = torch.einsum('pf,pkc->fkc', Wf, dBc).unsqueeze(1).to(wB.dtype) if ctx.needs_input_grad[3] else None
        gWi = torch.einsum('pkc,fkc->pf', dAc, A32)
        gWf = torch.einsum('pkc,fkc->pf', dBc, B32)
        gb = None
        if bias is not None:
            b32 = bias.detach().float().view(-1)
            gWi = gWi + torch.outer(dbx, b32)
            gWf = gWf + torch.outer(dbh, b32)
            if ctx.needs_input_grad[4]:
                gb = (Wi.t() @ dbx + Wf.t() @ dbh).view_as(bias).to(bias.dtype)
        g_mix_in = da_i.view(T * B, 2 * F).sum(dim=0).view_as(mix_in).to(mix_in.dtype) if ctx.needs_input_grad[5] else None
        g_w_in = gWi.view_as(w_in).to(w_in.dtype) if ctx.needs_input_grad[6] else None
        g_mix_f = da_f.view(T * B, 2 * F).sum(dim=0).view_as(mix_f).to(mix_f.dtype) if ctx.needs_input_grad[7] else None
        g_w_f = gWf.view_as(w_f).to(w_f.dtype) if ctx.needs_input_grad[8] else None
        return (None, None, gA, gB, gb, g_mix_in, g_w_in, g_mix_f, g_w_f,
                dgi if (gi is not None and ctx.needs_input_grad[9]) else None,
                dgf if (gf is not None and ctx.needs_input_grad[10]) else None, None, None, None, None)


def fused_edge_cell_train(X, h0, wA, wB, bias, graph, att_in, att_f, time_gates=None, negative_slope=0.2):
    """Training forward of the edge-gated (optionally time + edge gated) cell on the fused kernels; the time gates are autograd
    nodes of their own (_FusedTimeGate) and enter _FusedEdgeCell as differentiable [T][B] inputs."""
    require_device(X, h0, wA, wB, bias)
    with torch.no_grad():
        if time_gates is not None:
            xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0, graph, wA.shape[0], max(wA.shape[2], wB.shape[2]))
        else:
            xs, hs_all = fused_pack_inputs(X, h0, graph)
        hzero = fused_h0_zero_flag(h0)
    gi = gf = None
    if time_gates is not None:
        gi, gf = fused_train_time_gates(xs, hs_all[:1], X, h0, time_gates, graph, hzero, pending=pending)
        assert pending is None or pending.settled
    return _FusedEdgeCell.apply(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], gi, gf, graph, xs, hs_all, float(negative_slope))


def fused_x3_supported(graph, N, F, G, Kin, Kst, dtype, E=1, B=None, T=None):
    """fp32-accurate fused inference (gcrnn_fused_forward_x3): fp32 tensors, un-gated cell, N <= 1024 with N % 4 == 0, the fused
    shapes, and a UNIFORM-weight graph (all non-zeros equal: the drivers' W / lambda_max) with >= 16 padding rows."""
    if E != 1 or dtype != torch.float32 or N > int(lib.gcrnn_fused_padded_nodes()):
        return False
    Gp = fused_padded_inputs(F, G)
    if Gp is None:
        return False
    plan = graph.fused_plan_x3()
    if B is not None and T is not None:
        # limits of the x3 pack (gridDim.z = B * T) and of the 32-bit offsets into the three-plane arrays: such batches fall back to the
        # composed path instead of failing inside the forward (or, worse, inside the backward after the forward has run)
        if B * T > 65535 or 3 * B * plan['npad'] * max(F, Gp) * 2 > 2 ** 31 - 1:
            return False
    return plan.get('uniform_w', 0.0) != 0.0 and bool(lib.gcrnn_fused_x3_supported(int(N), int(F), int(Gp), int(max(Kin, Kst)), plan['entries']))


def time_fused_x3_kernel(X, h0, wA, wB, bias, graph, reps=3):
    """Average duration of ONE launch of the fp32-accurate step kernel (HIP events on the launch stream, inputs pre-packed)."""
    X, wA = fused_pad_operands(X, wA.detach())
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan_x3()
    npad, st, dev = plan['npad'], _stream(), X.device
    Xc, h0c = X.contiguous(), h0.contiguous()
    xs3 = torch.empty((T, 3, B, npad, G), dtype=torch.bfloat16, device=dev)
    h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    hs3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(Xc), _p(xs3), B, T, G, N, npad, st), 'pack_seq_x3')
    check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
    wAc, wBc = wA.float().contiguous(), wB.detach().float().contiguous()
    wp3 = torch.empty((3 * (F // 16) * K * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_fused_pack_weights_x3(_p(wAc), _p(wBc), _p(wp3), F, G, Kin, Kst, st), 'pack_weights_x3')
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    H = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        check(lib.gcrnn_fused_forward_x3(_p(xs3), _p(h03), _p(hs3), _p(wp3), _p(b32), *_wide_graph_args(plan),
                                         B, T, N, F, G, K, plan['uniform_w'], _p(H), 0, _p(plan.get('rank1_x3')), st),
              'fused_forward_x3')
    e1.record()
    torch.cuda.synchronize()
    return {'avg_us': 1e3 * e0.elapsed_time(e1) / (reps * T), 'launches': reps * T}


def fused_cell_forward_x3(X, h0, wA, wB, bias, graph, last_only=False, keep=False):
    """Un-gated GGCRNNCell forward to fp32 accuracy on the fused kernels (three bf16 planes per fp32 operand, six partial
    products per tap product on the bf16 matrix cores, fp32 hops / tanh). X: B x T x G x N fp32, h0: B x F x N fp32 ->
    H: B x T x F x N fp32 (B x 1 x F x N with last_only). No autograd graph here; keep: also returns the planes of the states
    hs3 [T][3][B][NPad][F] and the (channel-padded) X the kernels ran on -- what the fp32-accurate BPTT needs."""
    require_device(X, h0, wA, wB, bias)
    X, wA = fused_pad_operands(X, wA.detach())
    B, T, G, N = X.shape
    F = wA.shape[0]
    Kin, Kst = wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan_x3()
    npad = plan['npad']
    st = _stream()
    dev = X.device
    Xc, h0c = X.contiguous(), h0.contiguous()
    xs3 = torch.empty((T, 3, B, npad, G), dtype=torch.bfloat16, device=dev)
    h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    hs3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(Xc), _p(xs3), B, T, G, N, npad, st), 'pack_seq_x3')
    check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
    wAc, wBc = wA.float().contiguous(), wB.detach().float().contiguous()
    wp3 = torch.empty((3 * (F // 16) * K * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_fused_pack_weights_x3(_p(wAc), _p(wBc), _p(wp3), F, G, Kin, Kst, st), 'pack_weights_x3')
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    H = torch.empty((B, 1 if last_only else T, F, N), dtype=torch.float32, device=dev)
    check(lib.gcrnn_fused_forward_x3(_p(xs3), _p(h03), _p(hs3), _p(wp3), _p(b32), *_wide_graph_args(plan),
                                     B, T, N, F, G, K, plan['uniform_w'], _p(H),
                                     int(last_only), _p(plan.get('rank1_x3')), st), 'fused_forward_x3')
    if keep:
        return H, hs3, Xc
    return H


def fused_cell_forward_x3_gated(X, h0, wA, wB, bias, graph, gates, last_only=False):
    """Time-gated GGCRNNCell forward to fp32 accuracy on the fp32-accurate fused kernels (round 3; round 4: the gate cells run on the planes
    of X instead of per-item copies -- _x3_time_gated_forward). gates = {'in': (wA_g, wB_g, bias_g, lin_w, lin_b), 'forget': (...)} as in
    fused_cell_forward. X: B x T x G x N fp32, h0: B x F x N fp32 -> H: B x T x F x N fp32 (B x 1 x F x N with last_only). No autograd graph."""
    return _x3_time_gated_forward(X, h0, wA, wB, bias, graph, gates, keep=False, last_only=last_only)


def fused_x3_training_supported(graph, N, F, G, Kin, Kst, dtype, E=1, B=None, T=None):
    """fp32-accurate training of the un-gated cell on the fused kernels: the x3 forward's conditions, and the ADJOINT graph uniform
    too (a symmetric-support GSO like the drivers' W / lambda_max) with an image that fits next to the backward's two fp32 images."""
    if not fused_x3_supported(graph, N, F, G, Kin, Kst, dtype, E, B, T):
        return False
    pa = graph.fused_plan_x3(adjoint=True)
    Gp = fused_padded_inputs(F, G)
    return pa.get('uniform_w', 0.0) != 0.0 and bool(lib.gcrnn_fused_x3_training_supported(int(N), int(F), int(Gp), int(max(Kin, Kst)), int(pa['entries'])))


class _FusedCellX3(torch.autograd.Function):
    """Un-gated GGCRNNCell at fp32 accuracy on the fused kernels, forward AND BPTT (round 3): x3 forward; data chain on the x3 step
    kernel with the chain epilogue (gcrnn_fused_backward_data_x3); weight gradient on exact-fp32 matrix instructions
    (gcrnn_fused_backward_weight_f32). Gradients for the taps, the bias and h0; X gets none (the training loops never ask)."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, graph):
        H, hs3, Xp = fused_cell_forward_x3(X, h0, wA, wB, bias, graph, keep=True)
        ctx.save_for_backward(Xp, h0, wA, wB, bias, H, hs3)
        ctx.graph = graph
        ctx.G = X.shape[2]
        return H

    @staticmethod
    def backward(ctx, dH):
        Xp, h0, wA, wB, bias, H, hs3 = ctx.saved_tensors
        graph = ctx.graph
        if ctx.needs_input_grad[0]:
            raise GcrnnError('the fp32-accurate fused BPTT does not produce the gradient w.r.t. the input sequence X')
        B, T, Gp, N = Xp.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        plan = graph.fused_plan_x3(adjoint=True)
        npad, st, dev = plan['npad'], _stream(), Xp.device
        dHc = dH.float().contiguous()
        dH3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_pack_seq_major_x3(_p(dHc), _p(dH3), B, T, F, N, npad, st), 'pack_seq_x3')
        wBk = _pad_tap_count(wB.detach().float(), K)
        wp3T = _pack_state_taps_x3(wBk[:, 0].permute(2, 1, 0).contiguous(), K, st)      # [F_in][K][F_out]: transposed taps
        dpre3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        dh03 = torch.empty((3, B, npad, F), dtype=torch.bfloat16, device=dev) if ctx.needs_input_grad[1] else None
        check(lib.gcrnn_fused_backward_data_x3(_p(dH3), _p(hs3), _p(dpre3), _p(dh03), _p(wp3T), *_wide_graph_args(plan),
                                               B, T, N, F, K, plan['uniform_w'], _p(plan.get('rank1_x3')), st), 'fused_backward_data_x3')
        slots = int(lib.gcrnn_fused_wgrad_slots(T * B, F))
        dWp = torch.zeros((slots, F, K, F + Gp), dtype=torch.float32, device=dev)
        dbp = torch.zeros((slots, F), dtype=torch.float32, device=dev)
        h0c = h0.detach().float().contiguous()
        check(lib.gcrnn_fused_backward_weight_f32(_p(dpre3), _p(Xp), _p(H), _p(h0c), _p(dWp), _p(dbp), *_wide_graph_args(plan),
                                                  B, T, N, F, Gp, K, plan['uniform_w'], _p(plan.get('rank1_x3')), st), 'fused_backward_weight_f32')
        dW = dWp.sum(dim=0)                                                 # fixed order over the slots: bit-reproducible
        G = ctx.G
        gA = dW[:, :Kin, F:F + G].unsqueeze(1).to(wA.dtype) if ctx.needs_input_grad[2] else None
        gB = dW[:, :Kst, :F].unsqueeze(1).to(wB.dtype) if ctx.needs_input_grad[3] else None
        gb = dbp.sum(dim=0).view_as(bias).to(bias.dtype) if (bias is not None and ctx.needs_input_grad[4]) else None
        gh0 = None
        if dh03 is not None:
            gh0 = (dh03[2].float() + dh03[1].float() + dh03[0].float())[:, :N, :].permute(0, 2, 1).contiguous().to(h0.dtype)
        return None, gh0, gA, gB, gb, None


def fused_cell_train_x3(X, h0, wA, wB, bias, graph):
    """Training forward of the un-gated cell at fp32 accuracy on the fused kernels (fp32 tensors and parameters)."""
    require_device(X, h0, wA, wB, bias)
    return _FusedCellX3.apply(X, h0, wA, wB, bias, graph)


def _pack_state_taps_x3(w, K, st):
    """The x3 pack (three bf16 planes per tap) of a state-only operand: w [F][1][K][F] or [F][K][F], fp32 and contiguous."""
    F = w.shape[0]
    wp = torch.empty((3 * (F // 16) * K * (F // 32) * 64 * 8,), dtype=torch.bfloat16, device=w.device)
    check(lib.gcrnn_fused_pack_weights_x3(_p(w), _p(w), _p(wp), F, 0, K, K, st), 'pack_weights_x3')
    return wp


def _x3_planes_to_f32(p3):
    """[.., 3, B, NPad, C] bf16 planes -> fp32 (small to large: the sum is exact for planes cut from one fp32 value)."""
    return p3.select(-4, 2).float() + p3.select(-4, 1).float() + p3.select(-4, 0).float()


def _x3_item_slices(B, T):
    """(t0, nt) slices of the T*B items (t, b) that keep the x3 kernels' 32-bit buffer offsets and the pack's grid limit."""
    per = max(1, min(T, 2048 // B))
    return [(t0, min(per, T - t0)) for t0 in range(0, T, per)]


def fused_x3_time_training_supported(graph, N, F, G, Kin, Kst, dtype, E=1, B=None, T=None):
    """fp32-accurate training of the TIME-GATED cell on the fused kernels (ops.fused_cell_train_x3_gated): the un-gated x3 training's
    conditions; batches up to 2048 sequences (the gate cells run over slices of the T*B items)."""
    return (B is None or B <= 2048) and fused_x3_training_supported(graph, N, F, G, Kin, Kst, dtype, E, B, T)


def _x3_time_gated_forward(X, h0, wA, wB, bias, graph, gates, keep=False, last_only=False):
    """Forward of the time-gated cell at fp32 accuracy (reference graphML.py:2357-2374, 2420-2423): both gate cells as T x B one-step x3 cells
    that read (x_t, h0) on the planes of X (gcrnn_fused_gate_cells_x3), the Linear(F N -> 1) read-outs as GEMVs over their fp32 states, the
    recurrence as one scaled x3 step per launch -- gi (A(S)x_t + b) + gf (B(S)h_{t-1} + b) = A(S)(gi x_t) + B(S)(gf h_{t-1}) + (gi + gf) b, the
    operands scaled in fp32 while they are cut into planes (gcrnn_pack_seq_major_x3_ex). keep: what the BPTT needs."""
    require_device(X, h0, wA, wB, bias)
    Xp, wAp = fused_pad_operands(X, wA.detach())
    B, T, Gp, N = Xp.shape
    F, Kin, Kst = wAp.shape[0], wAp.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    plan = graph.fused_plan_x3()
    npad, st, dev = plan['npad'], _stream(), X.device
    Xp = Xp.float().contiguous()
    h0c = h0.detach().float().contiguous()
    # h0 == 0 (every training loop of the reference, train_rnn.py:256): the gate cells skip the state operand. A host-side read, so not under
    # stream capture (a captured step takes the general form: same results)
    hzero = False if torch.cuda.is_current_stream_capturing() else not bool(h0c.any())
    gargs = _wide_graph_args(plan)
    xs3 = torch.empty((T, 3, B, npad, Gp), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(Xp), _p(xs3), B, T, Gp, N, npad, st), 'pack_seq_x3')
    h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
    h3 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    gvals, cs = [], []
    for (wA_g, wB_g, bias_g, lin_w, lin_b) in (gates['in'], gates['forget']):
        Kg = max(wA_g.shape[2], wB_g.shape[2])
        wAg, wBg = wA_g.detach().float().contiguous(), wB_g.detach().float().contiguous()
        wpg = torch.empty((3 * (F // 16) * Kg * ((F + Gp) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_fused_pack_weights_x3(_p(wAg), _p(wBg), _p(wpg), F, Gp, wA_g.shape[2], wB_g.shape[2], st), 'pack_weights_x3')
        bg = bias_g.detach().float().contiguous().view(-1) if bias_g is not None else None
        c = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)          # the gate cells' states (training keeps them for their BPTT)
        check(lib.gcrnn_fused_gate_cells_x3(_p(xs3), _p(h03), _p(h3), _p(wpg), _p(bg), *gargs, B, T, N, F, Gp, Kg, plan['uniform_w'], _p(c), int(hzero), _p(plan.get('rank1_x3')), st),
              'fused_gate_cells_x3')
        logit = (c.view(B * T, F * N) @ lin_w.detach().float().reshape(-1)).view(B, T).t()
        if lin_b is not None:
            logit = logit + lin_b.detach().float().view(())
        gvals.append(torch.sigmoid(logit).contiguous())                          # [T][B]
        cs.append(c if keep else None)
        del c
    gi, gf = gvals
    xu3 = xs3 if (keep and Gp == F) else None                                               # (the backward's filter pass A(S) x_t reads the planes of X again)
    if xu3 is not None:
        xs3 = torch.empty_like(xu3)
    check(lib.gcrnn_pack_seq_major_x3_ex(_p(Xp), _p(xs3), B, T, Gp, N, npad, _p(gi), None, 0, 0, st), 'pack_seq_x3_ex')      # planes of gi x_t
    wAc, wBc = wAp.float().contiguous(), wB.detach().float().contiguous()
    wp3 = torch.empty((3 * (F // 16) * K * ((F + Gp) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_fused_pack_weights_x3(_p(wAc), _p(wBc), _p(wp3), F, Gp, Kin, Kst, st), 'pack_weights_x3')
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    bsc = (gi + gf).contiguous()
    H = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
    hs3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    for t in range(T):
        hprev = h0c if t == 0 else H[:, t - 1]
        check(lib.gcrnn_pack_seq_major_x3_ex(_p(hprev), _p(h3), B, 1, F, N, npad, _p(gf[t]), None, 0, 0 if t == 0 else T * F * N, st),
              'pack_seq_x3_ex')                                                                  # planes of gf_t h_{t-1}
        check(lib.gcrnn_fused_forward_x3_scaled(_p(xs3[t]), _p(h3), _p(hs3[t]), _p(wp3), _p(b32), _p(bsc[t]), *gargs, B, 1, N, F, Gp, K,
                                                plan['uniform_w'], _p(H[:, t]), T * F * N, _p(plan.get('rank1_x3')), st), 'fused_forward_x3_scaled')
    del xs3
    if last_only:
        return H[:, T - 1:].contiguous()
    return (H, Xp, h0c, hs3, gi, gf, cs[0], cs[1], hzero, xu3) if keep else H



def fused_node_x3_supported(graph, N, F, G, Kin, Kst, dtype, E=1, B=None, T=None):
    """Node-gated cell at fp32 accuracy on the x3 kernels (fused_node_cell_forward_x3): the x3 forward's conditions with G == F (the input
    filter runs as an F -> F x3 filter pass over the planes of X)."""
    return G == F and fused_x3_supported(graph, N, F, G, Kin, Kst, dtype, E, B, T) and not os.environ.get('GCRNN_NO_X3_NODE')


def fused_node_cell_forward_x3(X, h0, wA, wB, bias, graph, node_gates, time_gates=None, last_only=False):
    """Node-gated GGCRNNCell forward (optionally time-gated too) to fp32 accuracy on the fp32-accurate fused kernels (round 5; reference
    Utils/graphML.py:2379-2407, 2420-2423, in the drivers' precision class, kStepPredGRNNs.py:44):
        h_t = tanh( gi_t ni_t (.) (A(S) x_t + b) + gf_t nf_t (.) (B(S) h_{t-1} + b) )
    * both gate cells as T x B one-step x3 cells on the planes of X (gcrnn_fused_gate_cells_x3: they read (x_t, h0), never h_{t-1}), their
      F -> 1 graph filters on the fp32 any-shape filter kernels (lsigf_node_major), sigmoid;
    * A(S) x_t for all steps and B(S) h_{t-1} per step as x3 filter passes (gcrnn_fused_filter_x3: three bf16 planes per operand, exact fp32
      products on the matrix cores), the per-node gating and the tanh in fp32 between them -- the per-node gates multiply the filters'
      OUTPUTS, so (unlike the scalar time gates) they cannot be folded into the operands.
    node_gates = {'in': (wA_g, wB_g, bias_g, wf, bf), 'forget': (...)}, time_gates as in fused_cell_forward_x3_gated. X: B x T x G x N fp32 with
    G == F, h0: B x F x N fp32 -> H: B x T x F x N fp32 (B x 1 x F x N with last_only). Inference (no autograd graph)."""
    require_device(X, h0, wA, wB, bias)
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    assert G == F, 'the x3 filter pass takes F -> F filters'
    K = max(Kin, Kst)
    plan = graph.fused_plan_x3()
    npad, st, dev = plan['npad'], _stream(), X.device
    Xc = X.detach().float().contiguous()
    h0c = h0.detach().float().contiguous()
    hzero = False if torch.cuda.is_current_stream_capturing() else not bool(h0c.any())
    gargs = _wide_graph_args(plan)
    r1 = _p(plan.get('rank1_x3'))
    xs3 = torch.empty((T, 3, B, npad, G), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(Xc), _p(xs3), B, T, G, N, npad, st), 'pack_seq_x3')
    h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
    h3 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)

    def gate_cell_states(wA_g, wB_g, bias_g):
        Kg = max(wA_g.shape[2], wB_g.shape[2])
        wAg, wBg = wA_g.detach().float().contiguous(), wB_g.detach().float().contiguous()
        wpg = torch.empty((3 * (F // 16) * Kg * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_fused_pack_weights_x3(_p(wAg), _p(wBg), _p(wpg), F, G, wA_g.shape[2], wB_g.shape[2], st), 'pack_weights_x3')
        bg = bias_g.detach().float().contiguous().view(-1) if bias_g is not None else None
        c = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
        check(lib.gcrnn_fused_gate_cells_x3(_p(xs3), _p(h03), _p(h3), _p(wpg), _p(bg), *gargs, B, T, N, F, G, Kg, plan['uniform_w'], _p(c), int(hzero), r1, st),
              'fused_gate_cells_x3')
        return c

    # per-node gates [T][B][npad][1] fp32 (zero on the padding rows)
    Kf = node_gates['in'][3].shape[2]
    uw_f = graph.fused_plan().get('uniform_w', 0.0)      # (the x3 plan of a rank-1-weighted graph is its 0 / 1 pattern with uniform_w = 1: the gate filter reads the GSO itself)
    taps_first = (node_gates['forget'][3].shape[2] == Kf and not os.environ.get('GCRNN_NO_NODE_GATE_FILTER')
                  and bool(lib.gcrnn_node_gate_filter_supported(Kf, N, graph.fwd[0].nnz, uw_f)))
    if taps_first:
        # the F -> 1 filters taps-first (as the bf16 path): u_k = c w_k per node in fp32, then the K - 1 hops on ONE channel with the bias and the
        # sigmoid in the same pass (gcrnn_node_gate_filter_f32) -- the filter on the F-channel states cost half of this forward (34 of 69 ms)
        parts = torch.empty((T, B, 2, 1, Kf, N), dtype=torch.float32, device=dev)
        for gidx, name in enumerate(('in', 'forget')):
            wA_g, wB_g, bias_g, wf, bf = node_gates[name]
            c = gate_cell_states(wA_g, wB_g, bias_g)
            parts[:, :, gidx, 0] = torch.einsum('kf,btfn->tbkn', wf.detach().float()[0, 0], c)
            del c
        bfs = tuple(node_gates[name][4] for name in ('in', 'forget'))
        b2 = None
        if any(b is not None for b in bfs):
            b2 = torch.cat([(b.detach().float().reshape(1) if b is not None else torch.zeros(1, device=dev)) for b in bfs]).contiguous()
        csr = graph.fwd[0]
        ng2 = torch.empty((T, 2, B, N), dtype=torch.float32, device=dev)
        check(lib.gcrnn_node_gate_filter_f32(_p(parts), _p(ng2), T * B * 2, 1, Kf, N, 2, B, _p(csr.rowptr), _p(csr.col), _p(csr.val(torch.float32)), csr.nnz,
                                             uw_f, _p(b2), 1, st), 'node_gate_filter')
        del parts
        ngate = []
        for gidx in range(2):
            g = torch.zeros((T, B, npad, 1), dtype=torch.float32, device=dev)
            g[:, :, :N, 0] = ng2[:, gidx]
            ngate.append(g)
        del ng2
    else:
        ngate = []
        for name in ('in', 'forget'):
            wA_g, wB_g, bias_g, wf, bf = node_gates[name]
            c = gate_cell_states(wA_g, wB_g, bias_g)
            logit = lsigf_node_major(pack_node_major(c), wf.detach().float(), bf.detach().float() if bf is not None else None, graph, 1.0)      # [T][N][B][1]
            del c
            g = torch.zeros((T, B, npad, 1), dtype=torch.float32, device=dev)
            g[:, :, :N] = torch.sigmoid(logit).permute(0, 2, 1, 3)
            ngate.append(g)
            del logit
    ni, nf = ngate
    if time_gates is not None:
        for which, name in ((0, 'in'), (1, 'forget')):
            wA_g, wB_g, bias_g, lin_w, lin_b = time_gates[name]
            c = gate_cell_states(wA_g, wB_g, bias_g)
            logit = (c.view(B * T, F * N) @ lin_w.detach().float().reshape(-1)).view(B, T).t()
            if lin_b is not None:
                logit = logit + lin_b.detach().float().view(())
            tgv = torch.sigmoid(logit).contiguous().view(T, B, 1, 1)
            del c
            if which == 0:
                ni = ni * tgv
            else:
                nf = nf * tgv

    # F x 1 x k x F taps -> the x3 pack of a state-only operand with K taps
    wp3A, wp3B = (_pack_state_taps_x3(_pad_tap_count(w.detach().float(), K).contiguous(), K, st) for w in (wA, wB))
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    ya3 = torch.empty((3, B, npad, F), dtype=torch.bfloat16, device=dev)
    yb3 = torch.empty((3, B, npad, F), dtype=torch.bfloat16, device=dev)
    H = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h3), B, 1, F, N, npad, st), 'pack_seq_x3')
    for t in range(T):
        # both filter passes, then ONE pass: planes -> fp32, bias, per-node gating, tanh, the planes of h_t (the next step's operand) and H[:, t]
        check(lib.gcrnn_fused_filter_x3(_p(xs3[t]), _p(ya3), _p(wp3A), *gargs, B, N, F, K, plan['uniform_w'], r1, st), 'fused_filter_x3')      # A(S) x_t
        check(lib.gcrnn_fused_filter_x3(_p(h3[0]), _p(yb3), _p(wp3B), *gargs, B, N, F, K, plan['uniform_w'], r1, st), 'fused_filter_x3')       # B(S) h_{t-1}
        check(lib.gcrnn_x3_node_gate_step(_p(ya3), _p(yb3), _p(ni[t]), _p(nf[t]), _p(b32), _p(h3), _p(H[:, t]), T * F * N, B, N, npad, F, st), 'x3_node_gate_step')
    if last_only:
        return H[:, T - 1:].contiguous()
    return H


def fused_edge_cell_forward_x3(X, h0, wA, wB, bias, graph, att_in, att_f, time_gates=None, last_only=False):
    """Edge-gated GGCRNNCell forward (optionally time-gated too) to fp32 accuracy (round 5; reference Utils/graphML.py:2409-2416, 2420-2423,
    graphAttention :521-627):  h_t = tanh( gi_t GAT_in(A(S) x_t + b) + gf_t GAT_f(B(S) h_{t-1} + b) ).
    Both filters as x3 filter passes (gcrnn_fused_filter_x3: three bf16 planes per operand, exact fp32 products), the attentions on the fp32
    CSR edge-softmax kernels (att_in / att_f: callables on node-major [T][N][B][F] fp32 tensors, GraphAttentional.forward_node_major), the time
    gates' cells as one-step x3 cells. X: B x T x G x N fp32 with G == F, h0: B x F x N fp32 -> H: B x T x F x N fp32. Inference."""
    require_device(X, h0, wA, wB, bias)
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    assert G == F, 'the x3 filter pass takes F -> F filters'
    K = max(Kin, Kst)
    plan = graph.fused_plan_x3()
    npad, st, dev = plan['npad'], _stream(), X.device
    Xc = X.detach().float().contiguous()
    h0c = h0.detach().float().contiguous()
    gargs = _wide_graph_args(plan)
    r1 = _p(plan.get('rank1_x3'))
    xs3 = torch.empty((T, 3, B, npad, G), dtype=torch.bfloat16, device=dev)
    check(lib.gcrnn_pack_seq_major_x3(_p(Xc), _p(xs3), B, T, G, N, npad, st), 'pack_seq_x3')
    h3 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
    gi = gf = None
    if time_gates is not None:
        hzero = False if torch.cuda.is_current_stream_capturing() else not bool(h0c.any())
        h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
        gv = []
        for name in ('in', 'forget'):
            wA_g, wB_g, bias_g, lin_w, lin_b = time_gates[name]
            Kg = max(wA_g.shape[2], wB_g.shape[2])
            wAg, wBg = wA_g.detach().float().contiguous(), wB_g.detach().float().contiguous()
            wpg = torch.empty((3 * (F // 16) * Kg * ((F + G) // 32) * 64 * 8,), dtype=torch.bfloat16, device=dev)
            check(lib.gcrnn_fused_pack_weights_x3(_p(wAg), _p(wBg), _p(wpg), F, G, wA_g.shape[2], wB_g.shape[2], st), 'pack_weights_x3')
            bg = bias_g.detach().float().contiguous().view(-1) if bias_g is not None else None
            c = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
            check(lib.gcrnn_fused_gate_cells_x3(_p(xs3), _p(h03), _p(h3), _p(wpg), _p(bg), *gargs, B, T, N, F, G, Kg, plan['uniform_w'], _p(c), int(hzero), r1, st),
                  'fused_gate_cells_x3')
            logit = (c.view(B * T, F * N) @ lin_w.detach().float().reshape(-1)).view(B, T).t()
            if lin_b is not None:
                logit = logit + lin_b.detach().float().view(())
            gv.append(torch.sigmoid(logit).contiguous())      # [T][B]
            del c
        gi, gf = gv

    wp3A, wp3B = (_pack_state_taps_x3(_pad_tap_count(w.detach().float(), K).contiguous(), K, st) for w in (wA, wB))
    bvec = bias.detach().float().view(1, 1, F) if bias is not None else None
    y3 = torch.empty((3, B, npad, F), dtype=torch.bfloat16, device=dev)

    def filt(z3, wp):      # [3][B][npad][F] planes -> filter output + bias, node-major [1][N][B][F] fp32
        check(lib.gcrnn_fused_filter_x3(_p(z3), _p(y3), _p(wp), *gargs, B, N, F, K, plan['uniform_w'], r1, st), 'fused_filter_x3')
        y = torch.sum(y3, dim=0, dtype=torch.float32)      # (the three planes add up exactly in fp32)
        if bvec is not None:
            y = y + bvec
        return y[:, :N].permute(1, 0, 2).unsqueeze(0).contiguous()

    H = torch.empty((B, T, F, N), dtype=torch.float32, device=dev)
    hprev = h0c
    for t in range(T):
        gx = att_in(filt(xs3[t], wp3A))[0]                                   # [N][B][F]
        hp = hprev if hprev.is_contiguous() else hprev.contiguous()
        check(lib.gcrnn_pack_seq_major_x3(_p(hp), _p(h3), B, 1, F, N, npad, st), 'pack_seq_x3')
        gh = att_f(filt(h3[0], wp3B))[0]
        if gi is not None:
            pre = gi[t].view(1, B, 1) * gx + gf[t].view(1, B, 1) * gh
        else:
            pre = gx + gh
        H[:, t] = torch.tanh(pre).permute(1, 2, 0)
        hprev = H[:, t]
    if last_only:
        return H[:, T - 1:].contiguous()
    return H


class _FusedTimeCellX3(torch.autograd.Function):
    """Time-gated GGCRNNCell (the reference's default, Utils/graphML.py:2196, :2357-2374, :2420-2423) at fp32 accuracy on the fused kernels,
    forward AND BPTT (round 4). Forward: the two gate cells as T x B one-step x3 cells that all read h0 (gcrnn_fused_gate_cells_x3, on the
    planes of X) + the Linear(F N -> 1) read-out; the recurrence as scaled x3 steps (operands scaled while they are cut into planes), keeping
    the states' planes. Backward: the gated x3 data chain (gcrnn_fused_backward_data_x3_gated; the forget gate's gradient is read off the
    chain), d loss / d gi off one x3 filter pass A(S) x_t (gcrnn_fused_filter_x3 + gcrnn_x3_item_dots), the cell's weight gradient on
    exact-fp32 matrix instructions with the gates as operand weights (gcrnn_fused_backward_weight_f32_gated), and the gate cells' gradients:
    read-out by one GEMV over the kept gate states, taps / biases by the same weight-gradient kernel over all items (state operand = h0,
    skipped when it is zero). Gradients for every parameter; X and h0 get none (the training loops never ask: train_rnn.py:256 starts from
    zeros)."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gA_i, gB_i, gb_i, lw_i, lb_i, gA_f, gB_f, gb_f, lw_f, lb_f, graph):
        gates = {'in': (gA_i, gB_i, gb_i, lw_i, lb_i), 'forget': (gA_f, gB_f, gb_f, lw_f, lb_f)}
        H, Xp, h0c, hs3, gi, gf, c_i, c_f, hzero, xu3 = _x3_time_gated_forward(X, h0, wA, wB, bias, graph, gates, keep=True)
        ctx.save_for_backward(Xp, h0c, wA, wB, bias, gA_i, gB_i, gb_i, lw_i, lb_i, gA_f, gB_f, gb_f, lw_f, lb_f, H, hs3, gi, gf, c_i, c_f)
        ctx.graph, ctx.G, ctx.hzero, ctx.xu3 = graph, X.shape[2], hzero, xu3
        return H

    @staticmethod
    def backward(ctx, dH):
        (Xp, h0c, wA, wB, bias, gA_i, gB_i, gb_i, lw_i, lb_i, gA_f, gB_f, gb_f, lw_f, lb_f, H, hs3, gi, gf, c_i, c_f) = ctx.saved_tensors
        graph = ctx.graph
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise GcrnnError('the fp32-accurate fused BPTT of the time-gated cell does not produce the gradients w.r.t. X and h0')
        B, T, Gp, N = Xp.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        K = max(Kin, Kst)
        plan, pa = graph.fused_plan_x3(), graph.fused_plan_x3(adjoint=True)
        npad, st, dev = pa['npad'], _stream(), Xp.device
        gargs = _wide_graph_args(plan)
        aargs = _wide_graph_args(pa)
        nparts = (F // 16) * 8
        # ---- the gated data chain, d gf read off it ----
        dHc = dH.float().contiguous()
        dH3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_pack_seq_major_x3(_p(dHc), _p(dH3), B, T, F, N, npad, st), 'pack_seq_x3')
        h03 = torch.empty((1, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        check(lib.gcrnn_pack_seq_major_x3(_p(h0c), _p(h03), B, 1, F, N, npad, st), 'pack_seq_x3')
        wBk = _pad_tap_count(wB.detach().float(), K)
        wp3T = _pack_state_taps_x3(wBk[:, 0].permute(2, 1, 0).contiguous(), K, st)
        dpre3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        dh03 = torch.empty((3, B, npad, F), dtype=torch.bfloat16, device=dev)
        parts = torch.empty((T, B, nparts), dtype=torch.float32, device=dev)
        check(lib.gcrnn_fused_backward_data_x3_gated(_p(dH3), _p(hs3), _p(dpre3), _p(dh03), _p(wp3T), *aargs, B, T, N, F, K, pa['uniform_w'],
                                                     _p(gf), _p(h03), _p(parts), _p(pa.get('rank1_x3')), st), 'fused_backward_data_x3_gated')
        del dH3, dh03
        # ---- d gi = <A(S) x_t + b, dpre_t>: one filter pass per step over the planes of X (the input taps as an F -> F filter, zero columns
        # beyond G), dotted with dpre per item; the bias part <b, sum_n dpre_t> is shared with d gf ----
        bvec = bias.detach().float().contiguous().view(-1) if bias is not None else torch.zeros(F, dtype=torch.float32, device=dev)
        wAk = wA.detach().float()[:, 0]                                                              # [F][Kin][G]
        wAsq = torch.zeros((F, K, F), dtype=torch.float32, device=dev)
        wAsq[:, :Kin, :wAk.shape[2]] = wAk
        wp3A = _pack_state_taps_x3(wAsq, K, st)
        z3 = ctx.xu3
        ctx.xu3 = None
        if z3 is None:
            Xf = Xp if Gp == F else torch.nn.functional.pad(Xp, (0, 0, 0, F - Gp)).contiguous()
            z3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
            check(lib.gcrnn_pack_seq_major_x3(_p(Xf), _p(z3), B, T, F, N, npad, st), 'pack_seq_x3')
            del Xf
        y3 = torch.empty((T, 3, B, npad, F), dtype=torch.bfloat16, device=dev)
        for t in range(T):
            check(lib.gcrnn_fused_filter_x3(_p(z3[t]), _p(y3[t]), _p(wp3A), *gargs, B, N, F, K, plan['uniform_w'], _p(plan.get('rank1_x3')), st), 'fused_filter_x3')
        del z3
        dgi = torch.empty((T, B), dtype=torch.float32, device=dev)
        cb = torch.empty((T, B), dtype=torch.float32, device=dev)
        check(lib.gcrnn_x3_item_dots(_p(dpre3), _p(y3), _p(bvec), _p(dgi), _p(cb), B, T, npad, F, st), 'x3_item_dots')
        del y3
        dgi = dgi + cb
        dgf = parts.sum(dim=2) + cb
        # ---- the cell's taps and bias: exact-fp32 weight gradient, the gates as operand weights ----
        slots = int(lib.gcrnn_fused_wgrad_slots(T * B, F))
        dWp = torch.zeros((slots, F, K, F + Gp), dtype=torch.float32, device=dev)
        dbp = torch.zeros((slots, F), dtype=torch.float32, device=dev)
        check(lib.gcrnn_fused_backward_weight_f32_gated(_p(dpre3), _p(Xp), _p(H), _p(h0c), _p(dWp), _p(dbp), *aargs, B, T, N, F, Gp, K,
                                                        pa['uniform_w'], _p(gi), _p(gf), 0, _p(pa.get('rank1_x3')), st), 'fused_backward_weight_f32_gated')
        dW = dWp.sum(dim=0)
        G = ctx.G
        need = ctx.needs_input_grad
        gA = dW[:, :Kin, F:F + G].unsqueeze(1).to(wA.dtype) if need[2] else None
        gB = dW[:, :Kst, :F].unsqueeze(1).to(wB.dtype) if need[3] else None
        gb = dbp.sum(dim=0).view_as(bias).to(bias.dtype) if (bias is not None and need[4]) else None
        del dWp, dbp
        # ---- the gate cells: read-out by a GEMV over the kept states; taps / bias by the weight-gradient kernel over all items, the upstream
        # gradient d logit * w * (1 - c^2) formed while it is cut into planes (dpre3's buffer is reused) ----
        out = []
        for base, dgate, g, c, (wA_g, wB_g, bias_g, lin_w, lin_b) in ((5, dgi, gi, c_i, (gA_i, gB_i, gb_i, lw_i, lb_i)),
                                                                      (10, dgf, gf, c_f, (gA_f, gB_f, gb_f, lw_f, lb_f))):
            dlogit = (dgate * g * (1.0 - g)).contiguous()                                            # [T][B]
            Kg_in, Kg_st = wA_g.shape[2], wB_g.shape[2]
            Kg = max(Kg_in, Kg_st)
            Ggp = wA_g.shape[3]
            g_lw = (dlogit.t().reshape(1, B * T) @ c.view(B * T, F * N)).view_as(lin_w).to(lin_w.dtype) if need[base + 3] else None
            g_lb = dlogit.sum().view_as(lin_b).to(lin_b.dtype) if (lin_b is not None and need[base + 4]) else None
            g_wA = g_wB = g_b = None
            if need[base] or need[base + 1] or (bias_g is not None and need[base + 2]):
                lwv = lin_w.detach().float().contiguous().view(F, N)
                check(lib.gcrnn_pack_seq_major_x3_ex(_p(c), _p(dpre3), B, T, F, N, npad, _p(dlogit), _p(lwv), 1, 0, st), 'pack_seq_x3_ex')
                Xg = Xp if Ggp == Gp else Xp[:, :, :Ggp].contiguous()
                dWs = torch.zeros((slots, F, Kg, F + Ggp), dtype=torch.float32, device=dev)
                dbs = torch.zeros((slots, F), dtype=torch.float32, device=dev)
                check(lib.gcrnn_fused_backward_weight_f32_gated(_p(dpre3), _p(Xg), None, None if ctx.hzero else _p(h0c), _p(dWs), _p(dbs), *aargs,
                                                                B, T, N, F, Ggp, Kg, pa['uniform_w'], None, None, 1, _p(pa.get('rank1_x3')), st), 'fused_backward_weight_f32_gated')
                dWg, dbg = dWs.sum(dim=0), dbs.sum(dim=0)
                g_wA = dWg[:, :Kg_in, F:F + Ggp].unsqueeze(1).to(wA_g.dtype) if need[base] else None
                g_wB = dWg[:, :Kg_st, :F].unsqueeze(1).to(wB_g.dtype) if need[base + 1] else None
                g_b = dbg.view_as(bias_g).to(bias_g.dtype) if (bias_g is not None and need[base + 2]) else None
                del dWs, dbs
            out += [g_wA, g_wB, g_b, g_lw, g_lb]
        return (None, None, gA, gB, gb, *out, None)


def fused_cell_train_x3_gated(X, h0, wA, wB, bias, graph, gates):
    """Training forward of the TIME-GATED cell at fp32 accuracy on the fused kernels (fp32 tensors and parameters).
    gates = {'in': (wA_g, wB_g, bias_g, lin_w, lin_b), 'forget': (...)} as in fused_cell_forward (live parameters: they receive gradients)."""
    require_device(X, h0, wA, wB, bias)
    gi_, gf_ = gates['in'], gates['forget']
    return _FusedTimeCellX3.apply(X, h0, wA, wB, bias, *gi_, *gf_, graph)


def _fused_pack_state_taps(w, K, st):
    """Taps of ONE filter, w [F_out][1][k][C_in] (C_in == F_out on the fused path), packed as a state-only operand (G = 0)
    with K taps (zero beyond k)."""
    F, _, k, Cin = w.shape
    assert Cin == F
    wc = w.detach().contiguous()
    wpack = torch.empty(((F // 16) * K * (F // 32) * 64 * 8,), dtype=torch.bfloat16, device=w.device)
    check(lib.gcrnn_fused_pack_weights(dtype_code(wc.dtype), _p(wc), _p(wc), _p(wpack), F, 0, K, k, st), 'pack_weights')
    return wpack


def fused_pack_upstream(dH, graph, K):
    """dH [B][T][F][N] bf16 (user layout) -> (dHs [T][B][NPad][F] sequence-major, dH_user or None). On uniform-weight graphs only the
    last two steps are packed here and dH_user = dH: the BPTT launch that consumes dHs[t-1] lays out dHs[t-2] itself (inline pack,
    gcrnn_fused_backward_data_bf16 with dHuser_inline); otherwise the whole tensor is packed and dH_user is None."""
    B, T, F, N = dH.shape
    plan = graph.fused_plan(adjoint=True)
    npad = plan['npad']
    st = _stream()
    dHs = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=dH.device)
    if fused_inline_pack_ok(plan, N, F, F, K) and dH.data_ptr() % 16 == 0:
        check(lib.gcrnn_pack_seq_major_steps(_p(dH), _p(dHs), B, T, F, N, npad, max(T - 2, 0), T, 0, st), 'pack_seq_steps')
        return dHs, dH
    check(lib.gcrnn_pack_seq_major(_lib.BF16, _p(dH), _p(dHs), B, T, F, N, npad, None, st), 'pack_seq')
    return dHs, None


def fused_backward_data(dHs, hs, wB, graph, want_dh0=True, gf=None, h0s=None, bias=None, dH_user=None):
    """BPTT data-gradient chain of the fused cell. dHs, hs: [T][B][NPad][F] bf16 sequence-major (gradient of the loss
    w.r.t. every state; the states). gf: [T][B] fp32 forget gates of the time-gated cell or None.
    Returns (dpre [T][B][NPad][F] bf16, dh0 [B][NPad][F] bf16 or None), and with h0s ([1][B][NPad][F], the initial state)
    also d loss / d gf [T][B] fp32 = <B(S) h_{t-1} + bias, dpre_t>: its filter part is <h_{t-1}, adjoint chain of dpre_t>,
    read off the chain these launches evaluate anyway; the bias part is a column sum of dpre."""
    T, B, npad, F = hs.shape
    K = wB.shape[2]
    plan = graph.fused_plan(adjoint=True)
    st = _stream()
    wBt = _transposed_taps(wB)                                              # [F_in][1][K][F_out]
    dpre = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=hs.device)
    dh0 = torch.empty((B, npad, F), dtype=torch.bfloat16, device=hs.device) if want_dh0 else None
    plan16 = _adjoint_plan16(graph)                      # bf16 hop image, matrix-core sums (uniform graphs)
    pw = plan16 if plan16 is not None else _adjoint_plan16(graph, rank1=True)
    if pw is not None and F % 32 == 0 and not os.environ.get('GCRNN_NO_WIDE_CHAIN') and lib.gcrnn_fused_backward_data_wide_supported(
            B, T, graph.N, F, K, int(pw['entries']), float(pw.get('uniform_w', 0.0)), 3 if pw.get('rank1') else 1, 1 if dH_user is not None else 0):
        plan16 = pw
        # the whole chain (seed, T - 1 steps, d h0 / the forget gate's step 0) as ONE launch of the wide sequence-resident kernel
        wpw = _fused_pack_weights_wide(wBt.new_zeros((F, 1, K, 0)), wBt, plan16['uniform_w'], st)
        parts = torch.empty((T * B, (F // 32) * int(lib.gcrnn_fused_step_waves())), dtype=torch.float32, device=hs.device) if h0s is not None else None
        check(lib.gcrnn_fused_backward_data_wide_bf16(_p(dHs), _p(hs), _p(dpre), _p(dh0), _p(wpw), *_wide_graph_args(plan16),
                                                      B, T, graph.N, F, K, _p(gf), _p(h0s), _p(parts),
                                                      _p(dH_user), _p(plan16.get('rank1_a')), _p(plan16.get('rank1_b')), st), 'fused_backward_data_wide')
    else:
        wpack = _fused_pack_state_taps(wBt, K, st)
        parts = None
        if h0s is not None:
            parts = torch.empty((T * B, (F // 16) * int(lib.gcrnn_fused_step_waves())), dtype=torch.float32, device=hs.device)
        check(lib.gcrnn_fused_backward_data_bf16(_p(dHs), _p(hs), _p(dpre), _p(dh0), _p(wpack), *_fused_graph_args(plan16 or plan),
                                                 B, T, graph.N, F, K, _p(gf), _p(h0s), _p(parts), plan.get('uniform_w', 0.0), _p(dH_user),
                                                 1 if plan16 else 0, st),
              'fused_backward_data')
    return _chain_results(dpre, dh0, parts, h0s, bias)


def _chain_results(dpre, dh0, parts, h0s, bias):
    """What the data-gradient chains return: (dpre, dh0), and with h0s also d loss / d gf from the launches' partial sums."""
    if h0s is None:
        return dpre, dh0
    T, B = dpre.shape[0], dpre.shape[1]
    dgf = parts.sum(dim=1).view(T, B)
    if bias is not None:
        dgf = dgf + dpre.sum(dim=2, dtype=torch.float32) @ bias.detach().float().view(-1)
    return dpre, dh0, dgf


def fused_backward_data_head_plan(graph, B, T, N, F, K):
    """The adjoint bf16-image plan when gcrnn_fused_backward_data_wide_head_bf16 takes the problem (uniform-weight graph, persistent form),
    else None. GCRNN_NO_WIDE_CHAIN=1 switches the wide chain off altogether, this form included."""
    plan16 = _adjoint_plan16(graph)
    if plan16 is None or F % 32 != 0 or os.environ.get('GCRNN_NO_WIDE_CHAIN'):
        return None
    if not lib.gcrnn_fused_backward_data_wide_head_supported(B, T, N, F, K, int(plan16['entries']), float(plan16.get('uniform_w', 0.0)), 1):
        return None
    return plan16


def fused_backward_data_head(dy, w_head, hs, wB, graph, want_dh0=True, gf=None, h0s=None, bias=None):
    """fused_backward_data for cell + output head Linear(F -> 1) shared by all nodes: the upstream gradient of the states is
    dH[b][t][f][n] = bf16(w_head[f] dy[b][t][n]) -- what the head's backward kernel stores -- and enters as its factors dy [B][T][N] bf16 (user
    layout) and w_head [F] fp32; the ONE launch of the wide chain makes it in its epilogue (gcrnn_fused_backward_data_wide_head_bf16), so
    neither dH nor its sequence-major copy is allocated. Same results, bit for bit, as fused_backward_data on that dH. Raises where
    fused_backward_data_head_plan gives None."""
    T, B, npad, F = hs.shape
    K = wB.shape[2]
    N = graph.N
    plan16 = fused_backward_data_head_plan(graph, B, T, N, F, K)
    if plan16 is None:
        raise GcrnnError('fused_backward_data_head: the wide chain with the head\'s gradient does not take this problem '
                         '(fused_backward_data_head_plan)')
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and dy.numel() == B * T * N
    assert w_head.dtype == torch.float32 and w_head.is_contiguous() and w_head.numel() == F
    st = _stream()
    wBt = _transposed_taps(wB)                                              # [F_in][1][K][F_out]
    dpre = torch.empty((T, B, npad, F), dtype=torch.bfloat16, device=hs.device)
    dh0 = torch.empty((B, npad, F), dtype=torch.bfloat16, device=hs.device) if want_dh0 else None
    wpw = _fused_pack_weights_wide(wBt.new_zeros((F, 1, K, 0)), wBt, plan16['uniform_w'], st)
    parts = torch.empty((T * B, (F // 32) * int(lib.gcrnn_fused_step_waves())), dtype=torch.float32, device=hs.device) if h0s is not None else None
    check(lib.gcrnn_fused_backward_data_wide_head_bf16(_p(dy), _p(w_head), _p(hs), _p(dpre), _p(dh0), _p(wpw), *_wide_graph_args(plan16),
                                                       B, T, N, F, K, _p(gf), _p(h0s), _p(parts), st), 'fused_backward_data_wide_head')
    return _chain_results(dpre, dh0, parts, h0s, bias)


def fused_backward_weight(dpre, X, H, h0, graph, F, G, K, want_bias=False, gi=None, gf=None, h_is_h0=False, hzero=None):
    """dW [F][K][F+G] fp32 (columns: F state features, then G input features) from dpre (sequence-major bf16) and the
    user-layout bf16 tensors X [B][T][G][N], H [B][T][F][N] (forward output), h0 [B][F][N]. gi / gf [T][B] fp32: item
    (t, b) enters the input-filter columns with weight gi and the state-filter columns with gf (time-gated cell).
    h_is_h0: every item's state operand is h0 (gate sub-cells; H may be None).
    With want_bias also returns the bias gradient [F]: sum_{t,b} (gi + gf) sum_n dpre (the one bias enters both filters)."""
    T, B = dpre.shape[0], dpre.shape[1]
    # the kernel addresses dpre with 32-bit byte offsets: batches whose dpre passes 2 GiB (B = 512 at T = 32, F = 64) run as batch chunks -- sequences
    # are independent, the chunks' sums add (in chunk order: still bit-reproducible); the chunk of dpre is copied once to make it contiguous
    lim = (2 ** 31 - 1) // (T * dpre.shape[2] * F * 2)
    if B > lim >= 1:
        step = max(256 * (lim // 256), 1) if lim >= 256 else lim
        dW = dbs = None
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            r = fused_backward_weight(dpre[:, b0:b1].contiguous(), X[b0:b1], H[b0:b1] if H is not None else None, h0[b0:b1], graph, F, G, K, want_bias,
                                      gi[:, b0:b1].contiguous() if gi is not None else None, gf[:, b0:b1].contiguous() if gf is not None else None, h_is_h0, hzero)
            w, bsum = r if want_bias else (r, None)
            dW = w if dW is None else dW + w
            if want_bias:
                dbs = bsum if dbs is None else dbs + bsum
        return (dW, dbs) if want_bias else dW
    plan = graph.fused_plan(adjoint=True, kernel='wgrad')
    Xc, h0c = X.contiguous(), h0.contiguous()
    Hc = H.contiguous() if H is not None else None
    uw = 0.0 if os.environ.get('GCRNN_WGRAD_NO_UNIFORM') else plan.get('uniform_w', 0.0)      # env: A/B switch
    plan16 = None if uw == 0.0 else _adjoint_plan16(graph)      # bf16 hop image
    if plan16 is None and uw == 0.0 and not os.environ.get('GCRNN_WGRAD_NO_UNIFORM'):
        plan16 = _adjoint_plan16(graph, rank1=True)      # rank-1-weighted graph: kernel variant R1
        if plan16 is not None:
            uw = 1.0
    pl = plan16 or plan
    slots = int(lib.gcrnn_fused_wgrad_bf16_slots(T * B, F, K, pl['entries'], 1 if plan16 else 0))
    dWp = torch.zeros((slots, F, K, F + G), dtype=torch.float32, device=dpre.device)      # per-slot partial sums (plain stores)
    dbp = torch.zeros((slots, F), dtype=torch.float32, device=dpre.device) if want_bias else None
    check(lib.gcrnn_fused_backward_weight_bf16(_p(dpre), _p(Xc), _p(Hc), _p(h0c), _p(dWp),
                                               _p(dbp), _p(pl['tile_slots']), _p(pl['tile_off']), _p(pl['ell_val4']),
                                               _p(pl['ell_col4']), pl['entries'], B, T, graph.N, F, G, K,
                                               _p(gi), _p(gf), int(h_is_h0) | (2 if plan16 else 0), _p(hzero), uw,
                                               _p(plan16.get('rank1_a')) if plan16 else None, _p(plan16.get('rank1_b')) if plan16 else None, _stream()),
          'fused_backward_weight')
    dW = dWp.sum(dim=0)                                   # fixed order over the slots: bit-reproducible
    dbs = dbp.sum(dim=0) if want_bias else None
    return (dW, dbs) if want_bias else dW


def fused_gate_grad(zs, dpre, w, bias, graph, K):
    """d loss / d gate [T][B] fp32 of one filter of the time-gated cell: sum_{f,n} (w(S) z + bias) . dpre per item.
    zs: that filter's operand [T][B][NPad][C] bf16 sequence-major (h_{t-1}, or x_t), dpre: [T][B][NPad][F]; w: its taps
    F x 1 x k x C; bias F x 1 or None. C == F runs the operand alone; an input filter with C != F runs as [0 | x_t]."""
    T, B, npad, F = dpre.shape
    Cin = w.shape[3]
    plan = graph.fused_plan()
    plan16 = fused_img16_plan(graph, True, None)
    st = _stream()
    b32 = bias.detach().float().contiguous().view(-1) if bias is not None else None
    parts = torch.empty((T * B, (F // 16) * int(lib.gcrnn_fused_step_waves())), dtype=torch.float32, device=dpre.device)
    if Cin == F:
        wp = _fused_pack_state_taps(w, K, st)
        check(lib.gcrnn_fused_gate_grad_bf16(_p(zs), None, _p(dpre), _p(wp), _p(b32), _p(parts), *_fused_graph_args(plan16 or plan),
                                             B, T, graph.N, F, 0, K, plan.get('uniform_w', 0.0), 1 if plan16 else 0, st), 'fused_gate_grad')
    else:
        wd = w.detach()
        wz = wd.new_zeros((F, 1, K, F))
        wd = _pad_tap_count(wd, K)
        wp = _fused_pack_weights(wd, wz, st)
        zero_h = torch.zeros((1, npad, F), dtype=torch.bfloat16, device=dpre.device)
        check(lib.gcrnn_fused_gate_grad_bf16(_p(zero_h), _p(zs), _p(dpre), _p(wp), _p(b32), _p(parts), *_fused_graph_args(plan16 or plan),
                                             B, T, graph.N, F, Cin, K, plan.get('uniform_w', 0.0), 1 if plan16 else 0, st), 'fused_gate_grad')
    return parts.sum(dim=1).view(T, B)


def fused_training_supported(graph, N, F, G, Kin, Kst, E=1):
    """The fused BPTT needs the forward kernel's shapes, node-contiguous rows that are 16-byte aligned (N % 8 == 0)
    and the adjoint graph image next to the state and the transposed tile in LDS."""
    Gp = fused_padded_inputs(F, G)
    if E != 1 or N % 8 != 0 or Gp is None or not bool(lib.gcrnn_fused_supported(int(N), int(F), int(Gp), int(max(Kin, Kst)))):
        return False
    entries = graph.fused_plan(adjoint=True)['entries']
    return 65536 + 96 * entries + 16 * 1056 + 8 * 16 * 4 <= 160 * 1024


class _FusedTimeGate(torch.autograd.Function):
    """One time gate of the fused path with its BPTT (reference graphML.py:2357-2374): gate[t][b] = sigmoid(lin(vec(c_t))),
    c_t = tanh(A_g(S) x_t + B_g(S) h0 + 2 b_g).

    forward  = ONE pre-pass launch over all (t, b) that also stores c (bf16);
    backward = one in-place pass over c (read-out gradient + dpre_g = dlogit w (1 - c^2)), then the weight-gradient kernel
               over all items with h0 as every item's state operand. No gradient for X or h0 (the training loops start
               from h0 = 0 and never ask for either, train_rnn.py:247-276)."""

    @staticmethod
    def forward(ctx, xs, h0s, X, h0, wA_g, wB_g, bias_g, lin_w, lin_b, graph, hzero, pending=None):
        N = X.shape[3]
        gate, cs, gw = fused_time_gate(xs, h0s, wA_g, wB_g, bias_g, lin_w, lin_b, graph, N, store_states=True, hzero=hzero, pending=pending)
        ctx.save_for_backward(X, h0, wA_g, wB_g, bias_g, lin_w, lin_b, gate, cs, gw, hzero)
        ctx.graph = graph
        return gate

    @staticmethod
    def backward(ctx, dgate):
        X, h0, wA_g, wB_g, bias_g, lin_w, lin_b, gate, cs, gw, hzero = ctx.saved_tensors
        if getattr(ctx, 'consumed', False):
            raise GcrnnError('the fused time gate was already back-propagated: its saved states are turned into gradients in '
                             'place, so a second backward over the same graph (retain_graph) is not supported')
        ctx.consumed = True
        wx, wh = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if (wx or wh) and not fused_input_grad_ok(wA_g.shape[0], X.shape[2]):
            raise GcrnnError('the fused time gate produces gradients w.r.t. X or h0 only for G == F')
        res = _time_gate_backward(X, h0, wA_g, wB_g, bias_g, lin_w, lin_b, gate, cs, gw, hzero, ctx.graph, dgate, ctx.needs_input_grad[4:9], wx, wh)
        if wx or wh:
            return (None, None, res[0], res[1]) + res[2:] + (None, None, None)
        return (None, None, None, None) + res + (None, None, None)


def _time_gate_input_grads(X, h0, wA_g, wB_g, dpre_g, graph, want_x, want_h0):
    """d loss / d X and d loss / d h0 THROUGH a time gate (round 4; the reference's autograd gives both, graphML.py:2362, 2370: the gate cell
    reads (x_t, h0)): the gate cell's filters' adjoints on its dpre_g -- dX_t = sum_k (S^T)^k (dpre_g,t A_g,k), d h0 = sum_t sum_k (S^T)^k
    (dpre_g,t B_g,k) -- each ONE all-items launch of the filter-output pass on the adjoint graph with the transposed taps (G == F:
    fused_input_grad_ok). dpre_g [T][B][NPad][F] bf16. Returns (gX [B][T][G][N], gh0 [B][F][N]) in X's / h0's dtype, or None."""
    B, T, G, N = X.shape
    F, Kin, Kst = wA_g.shape[0], wA_g.shape[2], wB_g.shape[2]
    K = max(Kin, Kst)
    npad = dpre_g.shape[2]
    st = _stream()
    gX = gh0 = None
    if want_x:
        wAt = _transposed_taps(_pad_tap_count(wA_g, K))                           # [G][1][K][F]
        dxs = fused_filter_output(dpre_g, wAt, None, graph, K, N, adjoint=True)   # [T][B][NPad][G] bf16
        gX = _unpack_grad(dxs, B, T, G, N, st).to(X.dtype)
    if want_h0:
        wBt = _transposed_taps(_pad_tap_count(wB_g, K))
        dhs = fused_filter_output(dpre_g, wBt, None, graph, K, N, adjoint=True)   # every item's contribution to its sequence's h0
        dh = dhs.float().sum(dim=0).to(torch.bfloat16).unsqueeze(0).contiguous()  # [1][B][NPad][F]: fp32 sum over the T items of a sequence
        gh0 = _unpack_grad(dh, B, 1, F, N, st).view(B, F, N).to(h0.dtype)
    return gX, gh0


def _time_gate_backward(X, h0, wA_g, wB_g, bias_g, lin_w, lin_b, gate, cs, gw, hzero, graph, dgate, needs, want_x=False, want_h0=False):
    """BPTT of one time gate from its stored sub-cell states cs (turned into dpre_g IN PLACE): read-out gradient, then the weight-gradient
    kernel over all items with h0 as every item's state operand. Returns (gA, gB, gb, glw, glb); needs = which of them are wanted.
    want_x / want_h0: two more results in front, (gX, gh0) -- the gradients the gate hands to its inputs."""
    B, T, G, N = X.shape
    F, Kin, Kst = wA_g.shape[0], wA_g.shape[2], wB_g.shape[2]
    K = max(Kin, Kst)
    T_, B_, npad, _ = cs.shape
    items = T * B
    dlogit = (dgate.float() * gate * (1.0 - gate)).contiguous().view(-1)          # through the sigmoid
    slabs = int(lib.gcrnn_fused_gate_readout_slabs(items))
    dw_part = torch.empty((slabs, npad * F), dtype=torch.float32, device=X.device)
    # cs becomes dpre_g in place: a second backward through the same graph is not supported (retain_graph)
    check(lib.gcrnn_fused_gate_readout_backward_bf16(_p(cs), _p(dlogit), _p(gw), _p(dw_part), items, N, F, _stream()),
          'gate_readout_backward')
    dW, dbs = fused_backward_weight(cs, X, None, h0, graph, F, G, K, want_bias=True, h_is_h0=True, hzero=hzero)
    gA = dW[:, :Kin, F:].unsqueeze(1).to(wA_g.dtype) if needs[0] else None
    gB = dW[:, :Kst, :F].unsqueeze(1).to(wB_g.dtype) if needs[1] else None
    gb = dbs.view_as(bias_g).to(bias_g.dtype) if (bias_g is not None and needs[2]) else None
    glw = None
    if needs[3]:
        glw = dw_part.sum(dim=0).view(npad, F)[:N].t().reshape(1, F * N).to(lin_w.dtype)     # [N][F] -> vec over (f, n)
    glb = dlogit.sum().view(1).to(lin_b.dtype) if (lin_b is not None and needs[4]) else None
    if want_x or want_h0:
        return _time_gate_input_grads(X, h0, wA_g, wB_g, cs, graph, want_x, want_h0) + (gA, gB, gb, glw, glb)
    return gA, gB, gb, glw, glb


class _FusedTimeGatePair(torch.autograd.Function):
    """BOTH time gates of the fused path with their BPTT: forward = ONE pre-pass launch of the wide sequence-resident kernel over all (t, b)
    (fused_time_gate_pair: the two sub-cells as one cell of 2 F outputs; states of both stored), backward = _FusedTimeGate's, once per gate."""

    @staticmethod
    def forward(ctx, xs, h0s, X, h0, wA_i, wB_i, b_i, lw_i, lb_i, wA_f, wB_f, b_f, lw_f, lb_f, graph, hzero, pending=None):
        N = X.shape[3]
        gi, gf, (cs_i, gw_i), (cs_f, gw_f) = fused_time_gate_pair(xs, h0s, (wA_i, wB_i, b_i, lw_i, lb_i), (wA_f, wB_f, b_f, lw_f, lb_f), graph, N,
                                                                  store_states=True, hzero=hzero, pending=pending)
        ctx.save_for_backward(X, h0, wA_i, wB_i, b_i, lw_i, lb_i, wA_f, wB_f, b_f, lw_f, lb_f, gi, gf, cs_i, gw_i, cs_f, gw_f, hzero)
        ctx.graph = graph
        return gi, gf

    @staticmethod
    def backward(ctx, dgi, dgf):
        X, h0, wA_i, wB_i, b_i, lw_i, lb_i, wA_f, wB_f, b_f, lw_f, lb_f, gi, gf, cs_i, gw_i, cs_f, gw_f, hzero = ctx.saved_tensors
        if getattr(ctx, 'consumed', False):
            raise GcrnnError('the fused time gates were already back-propagated: their saved states are turned into gradients in '
                             'place, so a second backward over the same graph (retain_graph) is not supported')
        ctx.consumed = True
        wx, wh = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if (wx or wh) and not fused_input_grad_ok(wA_i.shape[0], X.shape[2]):
            raise GcrnnError('the fused time gates produce gradients w.r.t. X or h0 only for G == F')
        zi = torch.zeros_like(gi) if dgi is None else dgi
        zf = torch.zeros_like(gf) if dgf is None else dgf
        g_in = _time_gate_backward(X, h0, wA_i, wB_i, b_i, lw_i, lb_i, gi, cs_i, gw_i, hzero, ctx.graph, zi, ctx.needs_input_grad[4:9], wx, wh)
        g_f = _time_gate_backward(X, h0, wA_f, wB_f, b_f, lw_f, lb_f, gf, cs_f, gw_f, hzero, ctx.graph, zf, ctx.needs_input_grad[9:14], wx, wh)
        gX = gh0 = None
        if wx or wh:
            gX = (g_in[0] + g_f[0]) if wx else None
            gh0 = (g_in[1] + g_f[1]) if wh else None
            g_in, g_f = g_in[2:], g_f[2:]
        return (None, None, gX, gh0) + g_in + g_f + (None, None, None)


def fused_train_time_gates(xs, h0s, X, h0, gates, graph, hzero, pending=None):
    """The two differentiable time gates [T][B] of a training step: ONE pre-pass launch for the pair where the wide kernel takes the problem
    (uniform-weight graph, a batch that fills the chip), else one launch per gate. pending: the _PendingLayout of xs; the first launch settles it."""
    T, B, npad, G = xs.shape
    N = X.shape[3]
    gin, gfo = gates['in'], gates['forget']
    F = gin[0].shape[0]
    K = max(gin[0].shape[2], gin[1].shape[2])
    pair16 = None
    if gin[0].shape == gfo[0].shape and gin[1].shape == gfo[1].shape and gin[0].shape[3] == G and not os.environ.get('GCRNN_NO_GATE_PAIR_TRAIN'):
        pair16, _ = fused_gate_pair_plan(graph, B, T, N, F, G, K, pending is not None and not pending.settled)
    if pair16 is not None:
        return _FusedTimeGatePair.apply(xs, h0s, X, h0, *gin, *gfo, graph, hzero, pending)
    gi = _FusedTimeGate.apply(xs, h0s, X, h0, *gin, graph, hzero, pending)
    gf = _FusedTimeGate.apply(xs, h0s, X, h0, *gfo, graph, hzero)
    return gi, gf


class _FusedCell(torch.autograd.Function):
    """GGCRNNCell (un-gated, or time-gated with the gates as differentiable inputs) on the fused kernels, forward and BPTT
    (bf16 activations, fp32 or bf16 parameters).

    backward = pack(dH) -> data-gradient chain (T launches of the step kernel on the adjoint graph with transposed taps,
    the recurrent part scaled by the forget gate) -> ONE weight-gradient launch over all T*B items (item weights gi / gf)
    -> with gates:  d gf = <B(S)h_{t-1} + b, dpre_t> = <h_{t-1}, adjoint chain of dpre_t> + b . colsum(dpre_t) falls out of
    the data-gradient launches (adjoint identity); d gi = <A(S)x_t + b, dpre_t> is one gate-gradient pass over all items.
    The gradient w.r.t. X (no training loop of the reference asks for it, train_rnn.py:247-276, but its autograd gives it) is the
    input filter's adjoint on dpre, gi_t (S^T)^k (dpre_t A_k): ONE all-items launch of the filter-output pass on the adjoint graph with
    the transposed input taps (G == F; ops.fused_input_grad_ok)."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, graph, xs, hs_all):
        gv = (gi, gf) if gi is not None else None
        hs_all, plan, H = fused_cell_forward(X, h0, wA, wB, bias, graph, return_states=True, gate_values=gv,
                                             packed=(xs, hs_all) if xs is not None else None)
        ctx.save_for_backward(X, h0, wA, wB, bias, H, hs_all, gi, gf, xs)
        ctx.graph = graph
        ctx.npad = plan['npad']
        return H

    @staticmethod
    def backward(ctx, dH):
        X, h0, wA, wB, bias, H, hs_all, gi, gf, xs = ctx.saved_tensors
        graph = ctx.graph
        K = max(wA.shape[2], wB.shape[2])
        if ctx.needs_input_grad[0] and not fused_input_grad_ok(wA.shape[0], X.shape[2]):
            raise GcrnnError('the fused BPTT produces the gradient w.r.t. the input sequence X only for G == F')
        hs = hs_all[1:]
        gated = gi is not None
        if gated:
            gi, gf = gi.detach().float().contiguous(), gf.detach().float().contiguous()
        dH = dH.to(torch.bfloat16).contiguous()
        dHs, dHu = fused_pack_upstream(dH, graph, K)
        wBk = _pad_tap_count(wB, K)
        if gated and ctx.needs_input_grad[6]:
            chain = fused_backward_data(dHs, hs, wBk, graph, want_dh0=ctx.needs_input_grad[1], gf=gf,
                                        h0s=hs_all[:1], bias=bias, dH_user=dHu)
        else:
            chain = fused_backward_data(dHs, hs, wBk, graph, want_dh0=ctx.needs_input_grad[1], gf=gf if gated else None, dH_user=dHu)
        return _fused_cell_backward_tail(ctx.needs_input_grad, chain, X, h0, wA, wB, bias, H, gi, gf, xs, graph) + (None, None, None)


def _fused_cell_backward_tail(needs, chain, X, h0, wA, wB, bias, H, gi, gf, xs, graph):
    """Everything of the fused cell's BPTT behind the data-gradient chain (`chain` = its results: dpre, dh0s and, for the forget gates, dgf):
    the weight-gradient launch, d gi, d h0 and d X. needs[0:7]: which of (X, h0, wA, wB, bias, gi, gf) want a gradient; gi / gf: the detached
    fp32 gates [T][B] or None. Returns those seven gradients."""
    dpre, dh0s = chain[0], chain[1]
    dgf = chain[2] if len(chain) > 2 else None
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    K = max(Kin, Kst)
    st = _stream()
    gated = gi is not None
    want_b = bias is not None and needs[4]
    dW, dbs = fused_backward_weight(dpre, X, H, h0, graph, F, G, K, want_bias=True,
                                    gi=gi if gated else None, gf=gf if gated else None)       # [F][K][F+G], [F] fp32
    gA = dW[:, :Kin, F:].unsqueeze(1).to(wA.dtype) if needs[2] else None
    gB = dW[:, :Kst, :F].unsqueeze(1).to(wB.dtype) if needs[3] else None
    gb = dbs.view_as(bias).to(bias.dtype) if want_b else None
    dgi = None
    if gated and needs[5]:
        xsq = xs if xs is not None else fused_pack_inputs(X, h0, graph)[0]
        dgi = fused_gate_grad(xsq, dpre, wA, bias, graph, K)
    gh0 = None
    if needs[1]:
        gh0 = _unpack_grad(dh0s, B, 1, F, N, st).view(B, F, N).to(h0.dtype)
    gX = None
    if needs[0]:
        # dX_t = gi_t sum_k (dpre_t A_k) shifted k times by S^T: the input filter's adjoint, every item in one launch
        wAt = _transposed_taps(_pad_tap_count(wA, K))                             # [G][1][K][F]
        dxs = fused_filter_output(dpre, wAt, None, graph, K, N, adjoint=True)     # [T][B][NPad][G] bf16
        gX = _unpack_grad(dxs, B, T, G, N, st)
        if gated:
            gX = gX * gi.t().reshape(B, T, 1, 1).to(gX.dtype)
        gX = gX.to(X.dtype)
    return gX, gh0, gA, gB, gb, dgi, dgf


class _FusedCellHead(torch.autograd.Function):
    """_FusedCell followed by the output head Linear(F -> 1) shared by all nodes (the regression model's `multipMlp` head with one output) as ONE
    autograd node: y [B*T][1][N] bf16. The forward is the cell's training forward and the head's kernel on H, launch for launch what the two
    nodes run. The backward never materialises dH: the head's kernel gives d w_head / d b_head alone (no dH store), and the wide chain makes
    its upstream operand bf16(w_head[f] dy[n]) in its own epilogue (fused_backward_data_head) -- bit for bit the gradients of the two nodes,
    without dH [B][T][F][N], its sequence-major copy and the traffic of both."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, hw, hb, graph, xs, hs_all):
        gv = (gi, gf) if gi is not None else None
        hs_all, plan, H = fused_cell_forward(X, h0, wA, wB, bias, graph, return_states=True, gate_values=gv,
                                             packed=(xs, hs_all) if xs is not None else None)
        B, T, F, N = H.shape
        hwc = hw.contiguous()
        hbc = hb.contiguous() if hb is not None else None
        assert hbc is None or hbc.dtype == hwc.dtype
        y = torch.empty((B * T, 1, N), dtype=torch.bfloat16, device=H.device)
        check(lib.gcrnn_node_linear_bf16_forward(dtype_code(hwc.dtype), _p(H), _p(hwc), _p(hbc), _p(y), B * T, N, F, 1, _stream()),
              'node_linear_bf16_forward')
        ctx.save_for_backward(X, h0, wA, wB, bias, H, hs_all, gi, gf, xs, hwc)
        ctx.graph = graph
        ctx.has_head_bias = hb is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        X, h0, wA, wB, bias, H, hs_all, gi, gf, xs, hw = ctx.saved_tensors
        graph = ctx.graph
        B, T, F, N = H.shape
        K = max(wA.shape[2], wB.shape[2])
        if ctx.needs_input_grad[0] and not fused_input_grad_ok(F, X.shape[2]):
            raise GcrnnError('the fused BPTT produces the gradient w.r.t. the input sequence X only for G == F')
        gated = gi is not None
        if gated:
            gi, gf = gi.detach().float().contiguous(), gf.detach().float().contiguous()
        dyc = dy.to(torch.bfloat16).contiguous()
        # the head's parameter gradients: its backward kernel without the dH store (a null dh: the partial sums are the same)
        nb = int(lib.gcrnn_node_linear_bf16_blocks(B * T, N))
        pw = torch.empty((nb, 1, F), dtype=torch.float32, device=H.device)
        pb = torch.empty((nb, 1), dtype=torch.float32, device=H.device)
        check(lib.gcrnn_node_linear_bf16_backward(dtype_code(hw.dtype), _p(H), _p(hw), _p(dyc), None, _p(pw), _p(pb), B * T, N, F, 1,
                                                  _stream()), 'node_linear_bf16_backward')
        ghw = pw.sum(dim=0).to(hw.dtype) if ctx.needs_input_grad[7] else None
        ghb = pb.sum(dim=0).to(hw.dtype) if (ctx.has_head_bias and ctx.needs_input_grad[8]) else None
        w32 = hw.detach().float().reshape(-1).contiguous()
        wBk = _pad_tap_count(wB, K)
        want_dgf = gated and ctx.needs_input_grad[6]
        chain = fused_backward_data_head(dyc, w32, hs_all[1:], wBk, graph, want_dh0=ctx.needs_input_grad[1], gf=gf if gated else None,
                                         h0s=hs_all[:1] if want_dgf else None, bias=bias if want_dgf else None)
        return _fused_cell_backward_tail(ctx.needs_input_grad, chain, X, h0, wA, wB, bias, H, gi, gf, xs, graph) + (ghw, ghb, None, None, None)


def fused_input_grad_ok(F, G):
    """d loss / d X on the fused path: the adjoint of the input filter runs as a square (state-like) operand of the filter-output pass."""
    return int(F) == int(G)


def fused_cell_train(X, h0, wA, wB, bias, graph, gates=None):
    """Training forward of the fused cell. gates: None, or the time-gate sub-networks {'in': (wA_g, wB_g, bias_g, lin_w,
    lin_b), 'forget': (...)} (graphML.py:2248-2278): both gates are evaluated (and back-propagated) on the fused kernels and
    enter the cell as differentiable [T][B] inputs."""
    require_device(X, h0, wA, wB, bias)
    if gates is None:
        return _FusedCell.apply(X, h0, wA, wB, bias, None, None, graph, None, None)
    with torch.no_grad():
        xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0, graph, wA.shape[0], max(wA.shape[2], wB.shape[2]))
        hzero = fused_h0_zero_flag(h0)
    gi, gf = fused_train_time_gates(xs, hs_all[:1], X, h0, gates, graph, hzero, pending=pending)
    assert pending is None or pending.settled                   # (the first pre-pass laid out the rest of X)
    return _FusedCell.apply(X, h0, wA, wB, bias, gi, gf, graph, xs, hs_all)


def fused_cell_head_train_supported(graph, B, T, N, F, K, wdtype):
    """Cell + head Linear(F -> 1) trains as one autograd node (fused_cell_head_train): the head's bf16 kernels take (N, F, 1) with these
    parameters, and the wide chain takes the head's gradient in its factors (fused_backward_data_head_plan)."""
    return node_linear_supported(F, 1, torch.bfloat16, N, wdtype) and fused_backward_data_head_plan(graph, B, T, N, F, K) is not None


def fused_cell_head_train(X, h0, wA, wB, bias, graph, head_w, head_b, gates=None):
    """fused_cell_train followed by the output head Linear(F -> 1) shared by all nodes (head_w [1][F], head_b [1] or None; fp32 or bf16):
    y [B*T][1][N] bf16, the values node_linear gives on the cell's H. One autograd node whose backward skips dH (_FusedCellHead);
    the time gates enter as in fused_cell_train."""
    require_device(X, h0, wA, wB, bias, head_w)
    if gates is None:
        return _FusedCellHead.apply(X, h0, wA, wB, bias, None, None, head_w, head_b, graph, None, None)
    with torch.no_grad():
        xs, hs_all, pending = fused_pack_inputs_gated(X.contiguous(), h0, graph, wA.shape[0], max(wA.shape[2], wB.shape[2]))
        hzero = fused_h0_zero_flag(h0)
    gi, gf = fused_train_time_gates(xs, hs_all[:1], X, h0, gates, graph, hzero, pending=pending)
    assert pending is None or pending.settled                   # (the first pre-pass laid out the rest of X)
    return _FusedCellHead.apply(X, h0, wA, wB, bias, gi, gf, head_w, head_b, graph, xs, hs_all)


def fused_cell_train_with_gates(X, h0, wA, wB, bias, graph, gi, gf):
    """Training forward of the time-gated fused cell with the gates [T][B] computed elsewhere (any autograd graph)."""
    require_device(X, h0, wA, wB, bias, gi, gf)
    return _FusedCell.apply(X, h0, wA, wB, bias, gi, gf, graph, None, None)


# ------------------------------------------------------------------------------------------ small-graph persistent path
def small_supported(N, nnz, G, F, Kin, Kst, dtype, E=1):
    if E != 1 or dtype not in (torch.float32, torch.float64):
        return False
    return bool(lib.gcrnn_small_supported(dtype_code(dtype), int(N), int(nnz), int(G), int(F), int(Kin), int(Kst)))


def small_dense_supported(N, G, F, Kin, Kst, dtype, backward, gated):
    if dtype not in (torch.float32, torch.float64) or os.environ.get('GCRNN_SMALL_GATHER'):   # env: A/B against the gather kernels
        return False
    return bool(lib.gcrnn_small_dense_supported(dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst),
                                                int(backward), int(gated)))


def _gate_strides(g, B, T, N):
    """Element strides (b, t, n) with which the matrix-core kernels read a gate tensor: [T][B] scalar gates or [B][T][N]."""
    if g is None:
        return 0, 0, 0
    if g.dim() == 2:
        assert tuple(g.shape) == (T, B)
        return 1, B, 0
    assert tuple(g.shape) == (B, T, N)
    return T * N, N, 1


SMALL_STATES_ALL, SMALL_STATES_LAST, SMALL_STATES_NONE = 0, 1, 2      # gcrnn.h: GCRNN_SMALL_STATES_*


def _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, store, head=None):
    """The one forward launch of the matrix-core family: the recurrence, the states `store` asks for and the output of `head`. head: None,
    ('last', head_w [C][F N], head_b [C] or None) -- the read-out on the last state, logits [B][C] -- or ('node', node_w [O][F], node_b [O] or
    None) -- the per-node head on every state, Y [B][T][O][N] -- or ('gnn', head_w [K_o][F], head_b [1] or None, act) -- the one-layer
    graph-filter head on every state, Y [B][T][1][N], act a key of _GFL_ACTS -- or ('cls_gnn', head_w [K_o][F], head_b [1] or None, act,
    lin_w [C][N], lin_b [C] or None, V [B][N] to fill or None) -- that graph-filter head on the last state and a read-out Linear(N -> C)
    behind it, logits [B][C]. Returns (H or None, logits / Y or None). Entry point: no head
    and every state gcrnn_small_dense_forward; no head and the last state gcrnn_small_dense_forward_head without a read-out; 'last' the
    same entry with one; 'node' gcrnn_small_dense_forward_node_head; 'gnn' gcrnn_small_dense_forward_gnn_head; 'cls_gnn'
    gcrnn_small_dense_forward_cls_gnn_head. Every operand stays a local of this frame up to the launch (_small_dense_bptt)."""
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    dt, dev = X.dtype, X.device
    kind, hw, hb = head[:3] if head is not None else (None, None, None)
    assert head is not None or store != SMALL_STATES_NONE
    H = None if store == SMALL_STATES_NONE else torch.empty((B, T if store == SMALL_STATES_ALL else 1, F, N), dtype=dt, device=dev)
    out, NC = None, 0
    if head is not None:
        NC = hw.shape[0]
        assert tuple(hw.shape) == ((NC, F * N) if kind == 'last' else (NC, F)) and hw.dtype == dt
        assert hb is None or (hb.dtype == dt and hb.numel() == (1 if kind in ('gnn', 'cls_gnn') else NC))
        hw = hw.detach().contiguous()
        hb = hb.detach().contiguous() if hb is not None else None
        if kind == 'cls_gnn':
            lw, lb, V = head[4:7]
            NL = lw.shape[0]
            assert tuple(lw.shape) == (NL, N) and lw.dtype == dt and (lb is None or (lb.dtype == dt and lb.numel() == NL))
            assert V is None or (V.is_contiguous() and V.dtype == dt and tuple(V.shape) == (B, N))
            lw = lw.detach().contiguous()
            lb = lb.detach().contiguous() if lb is not None else None
            out = torch.empty((B, NL), dtype=dt, device=dev)
        else:
            out = torch.empty((B, NC) if kind == 'last' else (B, T, 1 if kind == 'gnn' else NC, N), dtype=dt, device=dev)
    bvec = bias.detach().contiguous().view(-1) if bias is not None else None
    if gi is not None:
        gi, gf = gi.detach().to(dt).contiguous(), gf.detach().to(dt).contiguous()
    Xc, h0c, wAc, wBc = X.detach().contiguous(), h0.detach().contiguous(), wA.detach().contiguous(), wB.detach().contiguous()
    Sd = graph.dense(dt)
    gs = _gate_strides(gi, B, T, N)
    assert gs == _gate_strides(gf, B, T, N)
    args = (dtype_code(dt), _p(Xc), _p(h0c), _p(wAc), _p(wBc), _p(bvec), _p(gi), _p(gf), _p(Sd))
    dims = (B, T, N, G, F, Kin, Kst, gs[0], gs[1], gs[2])
    if head is None and store == SMALL_STATES_ALL:
        name = 'small_dense_forward'
        args += (_p(H),) + dims
    elif kind == 'cls_gnn':
        name = 'small_dense_forward_cls_gnn_head'
        args += (_p(hw), _p(hb), _p(lw), _p(lb), _p(H), _p(V), _p(out)) + dims + (NC, NL, _GFL_ACTS[head[3]], store)
    else:
        name = {'node': 'small_dense_forward_node_head', 'gnn': 'small_dense_forward_gnn_head'}.get(kind, 'small_dense_forward_head')
        args += (_p(hw), _p(hb), _p(H), _p(out)) + dims + ((NC, _GFL_ACTS[head[3]], store) if kind == 'gnn' else (NC, store))
    check(getattr(lib, 'gcrnn_' + name)(*args, _stream()), name)
    return H, out


def small_cell_forward(X, h0, wA, wB, bias, graph, gi=None, gf=None, last_only=False):
    """Whole recurrence in one launch, one workgroup per sequence (small graphs). X: B x T x G x N, h0: B x F x N
    (user layout, fp32 / fp64) -> H: B x T x F x N. gi / gf: gates of the input / state filter or None: [T][B] scalars per
    sequence and step (time gating) or [B][T][N] per node (node gating, or the product of both; matrix-core kernels only).
    last_only: B x 1 x F x N, the last state -- the matrix-core kernel then stores that state alone (the gather family slices).
    Inference only."""
    require_device(X, h0, wA, wB, bias)
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    if small_dense_supported(N, G, F, Kin, Kst, X.dtype, backward=False, gated=gi is not None):
        return _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, SMALL_STATES_LAST if last_only else SMALL_STATES_ALL)[0]
    csr = graph.fwd[0]
    bvec = bias.detach().contiguous().view(-1) if bias is not None else None
    if gi is not None:
        gi, gf = gi.to(X.dtype).contiguous(), gf.to(X.dtype).contiguous()
    Xc, h0c, wAc, wBc, vals = X.contiguous(), h0.contiguous(), wA.contiguous(), wB.contiguous(), csr.val(X.dtype)
    assert gi is None or gi.dim() == 2, 'per-node gates need the matrix-core kernels (small_dense_supported)'
    H = torch.empty((B, T, F, N), dtype=X.dtype, device=X.device)
    check(lib.gcrnn_small_forward(dtype_code(X.dtype), _p(Xc), _p(h0c), _p(wAc),
                                  _p(wBc), _p(bvec), _p(gi), _p(gf), _p(csr.rowptr), _p(csr.col),
                                  _p(vals), _p(H), B, T, N, G, F, Kin, Kst, csr.nnz, _stream()),
          'small_forward')
    return H[:, -1:] if last_only else H


def small_training_supported(N, nnz, G, F, Kin, Kst, dtype, E=1):
    return small_supported(N, nnz, G, F, Kin, Kst, dtype, E) and bool(
        lib.gcrnn_small_backward_supported(dtype_code(dtype), int(N), int(nnz), int(G), int(F), int(Kin), int(Kst)))


def small_input_grad_supported(N, nnz, G, F, Kin, Kst, dtype, E=1, gated=False, node_gates=False):
    """The one-launch BPTT kernels also return dX for this shape (their dx variants): small_training_supported, and the family the
    backward pass runs on takes the variant -- the matrix-core family where its dx image fits in LDS (per-node gates run there only),
    else the gather family (same LDS image as its plain backward)."""
    if not small_training_supported(N, nnz, G, F, Kin, Kst, dtype, E):
        return False
    if small_dense_supported(N, G, F, Kin, Kst, dtype, backward=True, gated=gated):
        return bool(lib.gcrnn_small_dense_backward_dx_supported(dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst),
                                                                int(bool(gated))))
    return not node_gates


class _SmallCell(torch.autograd.Function):
    """Small-graph cell with BPTT: forward = one launch (small_cell_kernel), backward = one launch
    (small_cell_bwd_kernel). Gradients for the parameters, the time gates and h0, and -- on the kernels' dx variants, only when
    X wants one -- for X (small_input_grad_supported)."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H = small_cell_forward(X, h0, wA.detach(), wB.detach(), bias.detach() if bias is not None else None, graph,
                               gi.detach() if gi is not None else None, gf.detach() if gf is not None else None)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, gi, gf)
        ctx.graph = graph
        return H

    @staticmethod
    def backward(ctx, dH):
        X, h0, H, wA, wB, bias, gi, gf = ctx.saved_tensors
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        dt, dev = X.dtype, X.device
        fwd, adj = ctx.graph.fwd[0], ctx.graph.adj[0]
        dense = small_dense_supported(N, G, F, Kin, Kst, dt, backward=True, gated=gi is not None)
        scalar_gates = gi is not None and gi.dim() == 2
        want_dx, want_dh0 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if want_dx and not small_input_grad_supported(N, fwd.nnz, G, F, Kin, Kst, dt, ctx.graph.E, gated=gi is not None,
                                                      node_gates=gi is not None and not scalar_gates):
            raise GcrnnError('small_cell_train: no gradient for X at this shape (small_input_grad_supported)')
        if dense:
            return _small_dense_bptt(X, h0, H, wA, wB, bias, gi, gf, ctx.graph, want_dx, want_dh0, ('dH', dH.contiguous(), None)) + (None,)
        # the gather family: two slots per sequence, gate gradients [T][B] straight from the kernel
        pA = torch.empty((B, 2, F, Kin, G), dtype=dt, device=dev)
        pB = torch.empty((B, 2, F, Kst, F), dtype=dt, device=dev)
        pb = torch.empty((B, F), dtype=dt, device=dev)
        dgi = dgf = None
        if gi is not None:
            assert scalar_gates, 'per-node gates need the matrix-core kernels (small_dense_supported)'
            gi, gf = gi.to(dt).contiguous(), gf.to(dt).contiguous()
            dgi = torch.empty((T, B), dtype=dt, device=dev)
            dgf = torch.empty((T, B), dtype=dt, device=dev)
        dh0 = torch.empty_like(h0) if want_dh0 else None
        dX = torch.empty_like(X) if want_dx else None
        bvec = bias.detach().contiguous().view(-1) if bias is not None else None
        # every operand is a named local up to the launch (_small_dense_bptt): dH.contiguous(), a first-use adj.val(dt)
        dHc, wAc, wBc, fval, aval = dH.contiguous(), wA.contiguous(), wB.contiguous(), fwd.val(dt), adj.val(dt)
        name = 'small_backward_dx' if want_dx else 'small_backward'
        args = (dtype_code(dt), _p(X), _p(h0), _p(H), _p(dHc), _p(wAc), _p(wBc), _p(bvec), _p(gi), _p(gf), _p(fwd.rowptr), _p(fwd.col),
                _p(fval), _p(adj.rowptr), _p(adj.col), _p(aval), _p(pA), _p(pB), _p(pb), _p(dgi), _p(dgf), _p(dh0))
        check(getattr(lib, 'gcrnn_' + name)(*args, *((_p(dX),) if want_dx else ()), B, T, N, G, F, Kin, Kst, fwd.nnz, _stream()), name)
        dwA = pA.sum(dim=(0, 1)).view(F, 1, Kin, G)
        dwB = pB.sum(dim=(0, 1)).view(F, 1, Kst, F)
        db = pb.sum(dim=0).view(F, 1) if bias is not None else None
        return dX, dh0, dwA, dwB, db, dgi, dgf, None


def _small_dense_bptt(X, h0, H, wA, wB, bias, gi, gf, graph, want_dx, want_dh0, seed):
    """The one BPTT launch of the matrix-core family and its reductions, from the tensors the forward saved. seed: the upstream gradient
    (kind, gradient, head weight), each contiguous: ('dH', dH [B][T][F][N], None), ('dlogits', dlogits [B][C], head_w [C][F N]) -- the
    read-out on the last state -- or ('dY', dY [B][T][O][N], node_w [O][F]) -- the per-node head; for the last two the kernel forms dH
    itself; or ('dcls', dlogits [B][C], head_w [K_o][F], lin_w [C][N], V [B][N], act, dU [B][K_o][N]) -- the graph-filter head and read-out
    on the last state: the kernel forms dH_T from dlogits, lin_w, the forward's V and the head's taps, and fills the caller's dU.
    Entry point: 'dH' gcrnn_small_dense_backward, or gcrnn_small_dense_backward_dx with want_dx; 'dlogits'
    gcrnn_small_dense_backward_head and 'dY' gcrnn_small_dense_backward_node_head, 'dcls' gcrnn_small_dense_backward_cls_gnn_head, each
    with dX or NULL. The caller has asked whether the
    shape has a dx variant. Returns (dX, dh0, dwA, dwB, db, dgi, dgf); the gradients of a head's own parameters are the caller's.

    Every operand is a named local of this frame up to the launch: a temporary (wA.contiguous(), a first-use graph.dense(dt)) would be
    released -- and its block handed to the next allocation -- before the launch."""
    kind, g, hw = seed[:3]
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    dt, dev = X.dtype, X.device
    assert g.is_contiguous() and (hw is None or hw.is_contiguous())
    pA = torch.empty((B, 1, F, Kin, G), dtype=dt, device=dev)          # one slot per sequence, summed below
    pB = torch.empty((B, 1, F, Kst, F), dtype=dt, device=dev)
    pb = torch.empty((B, F), dtype=dt, device=dev)
    dgi = dgf = None
    scalar_gates = gi is not None and gi.dim() == 2
    if gi is not None:
        gi, gf = gi.to(dt).contiguous(), gf.to(dt).contiguous()
        dgi = torch.empty((B, T, N), dtype=dt, device=dev)
        dgf = torch.empty((B, T, N), dtype=dt, device=dev)
    dh0 = torch.empty_like(h0) if want_dh0 else None
    dX = torch.empty_like(X) if want_dx else None
    bvec = bias.detach().contiguous().view(-1) if bias is not None else None
    wAc, wBc, Sd = wA.contiguous(), wB.contiguous(), graph.dense(dt)
    gs = _gate_strides(gi, B, T, N)
    cell = (_p(wAc), _p(wBc), _p(bvec), _p(gi), _p(gf), _p(Sd), _p(pA), _p(pB), _p(pb), _p(dgi), _p(dgf), _p(dh0))
    dims = (B, T, N, G, F, Kin, Kst, gs[0], gs[1], gs[2])
    if kind == 'dH':
        name = 'small_dense_backward_dx' if want_dx else 'small_dense_backward'
        args = cell + ((_p(dX),) if want_dx else ()) + dims
    elif kind == 'dcls':
        lw, V, act, dU = seed[3:]
        assert lw.is_contiguous() and V.is_contiguous() and dU.is_contiguous() and tuple(dU.shape) == (B, hw.shape[0], N)
        name = 'small_dense_backward_cls_gnn_head'
        args = (_p(lw), _p(V), _p(hw)) + cell + (_p(dX), _p(dU)) + dims + (hw.shape[0], lw.shape[0], _GFL_ACTS[act])
    else:
        name = 'small_dense_backward_head' if kind == 'dlogits' else 'small_dense_backward_node_head'
        args = (_p(hw),) + cell + (_p(dX),) + dims + (hw.shape[0],)
    check(getattr(lib, 'gcrnn_' + name)(dtype_code(dt), _p(X), _p(h0), _p(H), _p(g), *args, _stream()), name)
    if scalar_gates:                                      # a scalar gate collects the gradients of all its nodes
        dgi, dgf = dgi.sum(dim=2).t(), dgf.sum(dim=2).t()
    dwA = pA.sum(dim=(0, 1)).view(F, 1, Kin, G)
    dwB = pB.sum(dim=(0, 1)).view(F, 1, Kst, F)
    db = pb.sum(dim=0).view(F, 1) if bias is not None else None
    return dX, dh0, dwA, dwB, db, dgi, dgf


def small_cell_train(X, h0, wA, wB, bias, graph, gi=None, gf=None):
    return _SmallCell.apply(X, h0, wA, wB, bias, gi, gf, graph)


# ---- the classification model on the matrix-core kernels: read-out Linear(F N -> C) on the last state inside the two launches
def small_head_supported(N, G, F, Kin, Kst, C, dtype, backward, gated, dx=False):
    """The matrix-core small-graph kernels take this cell with a read-out of C classes on its last state
    (gcrnn_small_dense_head_supported; GCRNN_SMALL_GATHER=1 answers no, as for small_dense_supported)."""
    if not small_dense_supported(N, G, F, Kin, Kst, dtype, backward, gated):
        return False
    return bool(lib.gcrnn_small_dense_head_supported(dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(C),
                                                     int(bool(backward)), int(bool(gated)), int(bool(dx))))


def _small_head_forward(X, h0, wA, wB, bias, graph, head_w, head_b, gi, gf, store):
    """_small_dense_forward with the read-out on the last state: (H or None, logits [B][C])."""
    return _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, store, ('last', head_w, head_b))


def _wants_grad(*operands):
    """Autograd is recording and one of these tensors (None among them: an absent one) wants a gradient."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in operands)


def _small_dense_cell_head(fn, head, X, h0, wA, wB, bias, graph, gi, gf):
    """The one decision of the four matrix-core heads (the edge family's: _small_edge_cell_head): where nothing wants a gradient the
    inference launch that stores no state, else the autograd node fn. head: _small_dense_forward's tuple, which names the head's
    parameters -- (kind, head_w, head_b[, act[, lin_w, lin_b, None]]); fn takes them in that order, then graph, then act."""
    params, act = head[1:3] + head[4:6], head[3:4]
    require_device(X, h0, wA, wB, bias, *params[::2])                 # (the weights; a bias lives where its weight does)
    if not _wants_grad(X, h0, wA, wB, bias, gi, gf, *params):
        return _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, SMALL_STATES_NONE, head)[1]
    return fn.apply(X, h0, wA, wB, bias, gi, gf, *params, graph, *act)


def _small_dense_head_bptt(ctx, entry, supported, head_shape, seed):
    """The backward of every matrix-core head node up to its own parameters: the dx question (supported, the node's shape query, with
    head_shape = (C,), (O,), (K_o,) or (K_o, C); entry: the public function the error names) and the one BPTT launch on what the forward
    saved, (dX, dh0, dwA, dwB, db, dgi, dgf). seed: _small_dense_bptt's (a seed that costs a launch, the graph-filter head's adjoint,
    has been issued by then: the route has asked the same question before the forward, so the error is a direct caller's)."""
    X, h0, H, wA, wB, bias, gi, gf = ctx.saved_tensors[:8]
    want_dx, want_dh0 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if want_dx and not supported(X.shape[3], X.shape[2], wA.shape[0], wA.shape[2], wB.shape[2], *head_shape, X.dtype, True, gi is not None,
                                 dx=True):
        raise GcrnnError('%s: no gradient for X at this shape (%s with dx)' % (entry, supported.__name__))
    return _small_dense_bptt(X, h0, H, wA, wB, bias, gi, gf, ctx.graph, want_dx, want_dh0, seed)


def _readout_grads(dlogits, h, want_w, want_b):
    """The own gradients of a read-out Linear on items h [B][...] from dlogits [B][C]: (d w = dlogits^T h [C][...flat] or None, d b, its
    column sums, or None). Library glue."""
    return (dlogits.t().mm(h.reshape(h.shape[0], -1)) if want_w else None, dlogits.sum(dim=0) if want_b else None)


def _node_head_grads(H, dU, w, want_w, want_b, bias_kernel, bias_level0):
    """The own gradients of a per-node linear head w [O][F] (contiguous) on the items H [R][F][N], from dU [R][O][N] (contiguous):
    (d w[o][f] = sum_{r,n} dU[r][o][n] H[r][f][n] or None, the bias gradient or None). No [R][F][N] temporary is made. The items: every
    stored state as it lies (R = B T), or a view of the last one (R = B), copied for the kernel. bias_kernel: the kernel also runs where
    the bias alone wants a gradient (the graph-filter heads), else that case is a sum of dU (the per-node heads). bias_level0: the bias
    gradient is level 0's sum alone, [1] (a graph filter's one bias), else all O column sums.

    The kernel is node_linear's own backward with dh = NULL: one pass over H and dU into per-block slots. The batched library product
    does the same in 20000 GEMMs of one row at B T = 20000 and measured 375 us against this kernel's 102 us WITH its dh store (fp32, the
    k-step driver's shape, T = 200: DESIGN 4.12); on R = B an einsum is ONE fp64 GEMM of 4 x 20 outputs over a contraction of B N = 5900
    -- a single serial tile, 0.13 ms of device time per step. Every operand of the launch is a named local of this frame
    (_small_dense_bptt), the copy of the last state included."""
    R, F, N = H.shape
    O, dt = dU.shape[1], H.dtype
    dw = db = None
    if (want_w or (bias_kernel and want_b)) and node_linear_supported(F, O, dt):
        Hc = H.contiguous()
        nblk = int(lib.gcrnn_node_linear_blocks(R, N))
        pw = torch.empty((nblk, O, F), dtype=dt, device=H.device)
        pb = torch.empty((nblk, O), dtype=dt, device=H.device)
        check(lib.gcrnn_node_linear_backward(dtype_code(dt), _p(Hc), _p(w), _p(dU), None, _p(pw), _p(pb), R, N, F, O, _stream()),
              'node_linear_backward')
        dw = pw.sum(dim=0) if want_w else None
        if want_b:
            db = pb[:, 0].sum(dim=0).view(1) if bias_level0 else pb.sum(dim=0)
    else:
        if want_w:                                        # F beyond node_linear's kernel: a batched product on views, [R][O][F] its only temporary
            dw = torch.bmm(dU, H.transpose(1, 2)).sum(0)
        if want_b:
            db = dU[:, 0].sum().view(1) if bias_level0 else dU.sum(dim=(0, 2))
    return dw, db


class _SmallCellHead(torch.autograd.Function):
    """Small-graph cell + Linear(F N -> C) on its last state as ONE autograd node. Forward: one launch that stores every state (BPTT
    reads them) and makes the logits. Backward: one BPTT launch seeded from dlogits inside the kernel (gcrnn_small_dense_backward_head:
    no dH [B][T][F][N] is allocated, zero-filled or read) plus the library product for the head's own parameters."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, head_w, head_b, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H, logits = _small_head_forward(X, h0, wA, wB, bias, graph, head_w, head_b, gi, gf, SMALL_STATES_ALL)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, gi, gf, head_w)
        ctx.graph, ctx.has_hb = graph, head_b is not None
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        H, head_w = ctx.saved_tensors[2], ctx.saved_tensors[8]
        dlc = dlogits.contiguous()
        grads = _small_dense_head_bptt(ctx, 'small_cell_classify', small_head_supported, (head_w.shape[0],),
                                       ('dlogits', dlc, head_w.detach().contiguous()))
        return grads + _readout_grads(dlc, H[:, -1], ctx.needs_input_grad[7], ctx.has_hb and ctx.needs_input_grad[8]) + (None,)


def small_cell_classify(X, h0, wA, wB, bias, graph, head_w, head_b, gi=None, gf=None):
    """The small-graph cell followed by Linear(F N -> C) on its last state (head_w [C][F*N], head_b [C] or None, the states' dtype):
    logits [B][C]. Where nothing wants a gradient it is one launch that stores no state; otherwise one autograd node (_SmallCellHead)
    with gradients for X (only where wanted: small_head_supported with dx), h0, the taps, the bias, the gates and the head. Shapes:
    small_head_supported."""
    return _small_dense_cell_head(_SmallCellHead, ('last', head_w, head_b), X, h0, wA, wB, bias, graph, gi, gf)


# ---- the regression model on the matrix-core kernels: per-node head Linear(F -> O) on every state inside the two launches
def small_node_head_supported(N, G, F, Kin, Kst, O, dtype, backward, gated, dx=False):
    """The matrix-core small-graph kernels take this cell with a per-node head of O outputs on every state
    (gcrnn_small_dense_node_head_supported; GCRNN_SMALL_GATHER=1 answers no, as for small_dense_supported). backward: the training step,
    i.e. the forward launch with the head's LDS share and the BPTT launch."""
    if not small_dense_supported(N, G, F, Kin, Kst, dtype, backward, gated):
        return False
    shape = (dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(O))
    if not lib.gcrnn_small_dense_node_head_supported(*shape, 0, int(bool(gated)), 0):
        return False
    return not backward or bool(lib.gcrnn_small_dense_node_head_supported(*shape, 1, int(bool(gated)), int(bool(dx))))


def _small_node_head_forward(X, h0, wA, wB, bias, graph, node_w, node_b, gi, gf, store):
    """_small_dense_forward with the per-node head on every state: (H or None, Y [B][T][O][N])."""
    return _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, store, ('node', node_w, node_b))


class _SmallCellNodeHead(torch.autograd.Function):
    """Small-graph cell + Linear(F -> O) shared by all nodes on every state as ONE autograd node. Forward: one launch that stores every
    state (BPTT reads them) and makes Y. Backward: one BPTT launch that forms dH_t = node_w^T dY_t inside the kernel
    (gcrnn_small_dense_backward_node_head: no dH [B][T][F][N] is allocated, written or read) plus the library products for the head's own
    parameters."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, node_w, node_b, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H, Y = _small_node_head_forward(X, h0, wA, wB, bias, graph, node_w, node_b, gi, gf, SMALL_STATES_ALL)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, gi, gf, node_w)
        ctx.graph, ctx.has_nb = graph, node_b is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, node_w = ctx.saved_tensors[2], ctx.saved_tensors[8]
        B, T, F, N = H.shape
        O = node_w.shape[0]
        dYc, nw = dY.contiguous(), node_w.detach().contiguous()
        grads = _small_dense_head_bptt(ctx, 'small_cell_regress', small_node_head_supported, (O,), ('dY', dYc, nw))
        return grads + _node_head_grads(H.view(B * T, F, N), dYc.view(B * T, O, N), nw, ctx.needs_input_grad[7],
                                        ctx.has_nb and ctx.needs_input_grad[8], bias_kernel=False, bias_level0=False) + (None,)


def small_cell_regress(X, h0, wA, wB, bias, graph, node_w, node_b, gi=None, gf=None):
    """The small-graph cell followed by Linear(F -> O) shared by all nodes on every state (node_w [O][F], node_b [O] or None, the states'
    dtype): Y [B][T][O][N]. Where nothing wants a gradient it is one launch that stores no state; otherwise one autograd node
    (_SmallCellNodeHead) with gradients for X (only where wanted: small_node_head_supported with dx), h0, the taps, the bias, the gates
    and the head. Shapes: small_node_head_supported."""
    return _small_dense_cell_head(_SmallCellNodeHead, ('node', node_w, node_b), X, h0, wA, wB, bias, graph, gi, gf)


# ---- the regression model's Selection-GNN head on the matrix-core kernels: GraphFilter(F -> 1, K_o) + activation on every state inside the
# forward launch; backward = the head's adjoint kernel + the per-node head's BPTT launch fed dU
def small_gnn_head_supported(N, G, F, Kin, Kst, K_o, dtype, backward, gated, dx=False, E=1):
    """The matrix-core small-graph kernels take this cell with a one-layer graph-filter head of K_o taps and one output feature on every
    state (gcrnn_small_dense_gnn_head_supported; E = 1, fp32 / fp64; GCRNN_SMALL_GATHER=1 answers no, as for small_dense_supported).
    backward: the training step, i.e. the forward launch with the head's LDS share, the adjoint kernel and the BPTT launch."""
    if E != 1 or not small_dense_supported(N, G, F, Kin, Kst, dtype, backward, gated):
        return False
    shape = (dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(K_o))
    if not lib.gcrnn_small_dense_gnn_head_supported(*shape, 0, int(bool(gated)), 0):
        return False
    return not backward or bool(lib.gcrnn_small_dense_gnn_head_supported(*shape, 1, int(bool(gated)), int(bool(dx))))


def small_gnn_head_adjoint(dY, Y, graph, K_o, act, out=None):
    """dU [B][T][K_o][N] of the graph-filter head from dY and the stored Y, both [B][T][1][N]: dU_0 = dY . act'(Y), dU_k = dU_{k-1} S^T
    (gcrnn_small_gnn_head_adjoint). out: a contiguous buffer to fill (every element is written), else a new one."""
    B, T, _, N = Y.shape
    dt = Y.dtype
    dYc, Yc, Sd = dY.contiguous(), Y.contiguous(), graph.dense(dt)
    assert dYc.dtype == dt and tuple(dYc.shape) == (B, T, 1, N)
    dU = out if out is not None else torch.empty((B, T, K_o, N), dtype=dt, device=Y.device)
    assert dU.is_contiguous() and dU.dtype == dt and tuple(dU.shape) == (B, T, K_o, N)
    check(lib.gcrnn_small_gnn_head_adjoint(dtype_code(dt), _p(dYc), _p(Yc), _p(Sd), _p(dU), B * T, N, K_o, _GFL_ACTS[act], _stream()),
          'small_gnn_head_adjoint')
    return dU


class _SmallCellGnnHead(torch.autograd.Function):
    """Small-graph cell + GraphFilter(F -> 1, K_o) + activation on every state as ONE autograd node. Forward: one launch that stores every
    state (BPTT reads them) and makes Y. Backward: the head's adjoint kernel (dU [B][T][K_o][N], K_o / F of a dH), then the per-node head's
    BPTT launch with node_w = head_w and dY := dU (gcrnn_small_dense_backward_node_head forms dH_t = sum_k w_k (x) dU_k itself: no dH
    [B][T][F][N] is allocated, written or read) and node_linear's backward kernel on (H, dU) for the head's own parameters."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, head_w, head_b, graph, act):
        X, h0 = X.contiguous(), h0.contiguous()
        H, Y = _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, SMALL_STATES_ALL, ('gnn', head_w, head_b, act))
        ctx.save_for_backward(X, h0, H, wA, wB, bias, gi, gf, head_w, Y)
        ctx.graph, ctx.has_hb, ctx.act = graph, head_b is not None, act
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, head_w, Y = ctx.saved_tensors[2], ctx.saved_tensors[8], ctx.saved_tensors[9]
        B, T, F, N = H.shape
        Ko = head_w.shape[0]
        dU, hw = small_gnn_head_adjoint(dY.to(H.dtype), Y, ctx.graph, Ko, ctx.act), head_w.detach().contiguous()
        grads = _small_dense_head_bptt(ctx, 'small_cell_regress_gnn', small_gnn_head_supported, (Ko,), ('dY', dU, hw))
        # the per-node head's sums with O = K_o on (H, dU); the bias is level 0's
        return grads + _node_head_grads(H.view(B * T, F, N), dU.view(B * T, Ko, N), hw, ctx.needs_input_grad[7],
                                        ctx.has_hb and ctx.needs_input_grad[8], bias_kernel=True, bias_level0=True) + (None, None)


def small_cell_regress_gnn(X, h0, wA, wB, bias, graph, head_w, head_b, act=None, gi=None, gf=None):
    """The small-graph cell followed by one graph-filter layer of K_o taps and one output feature on every state (head_w [K_o][F] =
    GraphFilter.weight[0, 0], head_b [1] or None, the states' dtype; act in (None, 'relu', 'tanh', 'sigmoid')):
    Y[b][t][0] = act(sum_k head_w[k] (h_t S^k) + head_b), [B][T][1][N] -- the values ops.graph_filter_layer gives on the cell's H, in
    another summation order. Where nothing wants a gradient it is one launch that stores no state; otherwise one autograd node
    (_SmallCellGnnHead) with gradients for X (only where wanted: small_gnn_head_supported with dx), h0, the taps, the bias, the gates and
    the head. Shapes: small_gnn_head_supported."""
    assert act in _GFL_ACTS, act
    return _small_dense_cell_head(_SmallCellGnnHead, ('gnn', head_w, head_b, act), X, h0, wA, wB, bias, graph, gi, gf)


# ---- the classification model's Selection-GNN head on the matrix-core kernels: GraphFilter(F -> 1, K_o) + activation + Linear(N -> C) on
# the last state inside the forward launch; the BPTT launch seeds itself from dlogits and writes the head's adjoint levels dU
def small_cls_gnn_head_supported(N, G, F, Kin, Kst, K_o, C, dtype, backward, gated, dx=False, E=1):
    """The matrix-core small-graph kernels take this cell with a one-layer graph-filter head of K_o taps and one output feature on its
    last state and a read-out of C classes behind it (gcrnn_small_dense_cls_gnn_head_supported; E = 1, fp32 / fp64; GCRNN_SMALL_GATHER=1
    answers no, as for small_dense_supported). backward: the training step, i.e. the forward launch with the head's LDS share and the
    BPTT launch."""
    if E != 1 or not small_dense_supported(N, G, F, Kin, Kst, dtype, backward, gated):
        return False
    shape = (dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(K_o), int(C))
    if not lib.gcrnn_small_dense_cls_gnn_head_supported(*shape, 0, int(bool(gated)), 0):
        return False
    return not backward or bool(lib.gcrnn_small_dense_cls_gnn_head_supported(*shape, 1, int(bool(gated)), int(bool(dx))))


class _SmallCellClsGnnHead(torch.autograd.Function):
    """Small-graph cell + GraphFilter(F -> 1, K_o) + activation + Linear(N -> C) on its last state as ONE autograd node. Forward: one
    launch that stores every state (BPTT reads them), the head's output V [B][N] and the logits. Backward: one BPTT launch seeded from
    dlogits inside the kernel (gcrnn_small_dense_backward_cls_gnn_head: no dH [B][T][F][N] and no buffer with a T in its shape is
    allocated, and no adjoint kernel runs), which also writes dU [B][K_o][N]; the head's own parameters take library products of
    dlogits, V, dU and the last state. No host synchronisation."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, gi, gf, head_w, head_b, lin_w, lin_b, graph, act):
        X, h0 = X.contiguous(), h0.contiguous()
        V = torch.empty((X.shape[0], X.shape[3]), dtype=X.dtype, device=X.device)
        H, logits = _small_dense_forward(X, h0, wA, wB, bias, graph, gi, gf, SMALL_STATES_ALL, ('cls_gnn', head_w, head_b, act, lin_w, lin_b, V))
        ctx.save_for_backward(X, h0, H, wA, wB, bias, gi, gf, head_w, lin_w, V)
        ctx.graph, ctx.has_hb, ctx.has_lb, ctx.act = graph, head_b is not None, lin_b is not None, act
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        H, head_w, lin_w, V = ctx.saved_tensors[2], ctx.saved_tensors[8], ctx.saved_tensors[9], ctx.saved_tensors[10]
        B, N, Ko, C, dt = V.shape[0], V.shape[1], head_w.shape[0], lin_w.shape[0], H.dtype
        dlc, hw, lw = dlogits.to(dt).contiguous(), head_w.detach().contiguous(), lin_w.detach().contiguous()
        dU = torch.empty((B, Ko, N), dtype=dt, device=H.device)
        grads = _small_dense_head_bptt(ctx, 'small_cell_classify_gnn', small_cls_gnn_head_supported, (Ko, C),
                                       ('dcls', dlc, hw, lw, V, ctx.act, dU))
        # the per-node head's sums with O = K_o on the B items of the last state (no buffer with a T in its shape), the bias level 0's;
        # d lin_w = dlogits^T V, d lin_b its column sums, as the MLP heads everywhere
        need = ctx.needs_input_grad
        return grads + _node_head_grads(H[:, -1], dU, hw, need[7], ctx.has_hb and need[8], bias_kernel=True, bias_level0=True) + \
            _readout_grads(dlc, V, need[9], ctx.has_lb and need[10]) + (None, None)


def small_cell_classify_gnn(X, h0, wA, wB, bias, graph, head_w, head_b, lin_w, lin_b, act=None, gi=None, gf=None):
    """The small-graph cell followed, on its last state, by one graph-filter layer of K_o taps and one output feature and a
    Linear(N -> C) (head_w [K_o][F] = GraphFilter.weight[0, 0], head_b [1] or None, lin_w [C][N], lin_b [C] or None, the states' dtype;
    act in (None, 'relu', 'tanh', 'sigmoid')): logits[b] = lin_w act(sum_k head_w[k] (h_T S^k) + head_b) + lin_b, [B][C] -- the values
    ops.graph_filter_layer and nn.Linear give on the cell's last state, in another summation order. Where nothing wants a gradient it
    is one launch that stores no state; otherwise one autograd node (_SmallCellClsGnnHead) with gradients for X (only where wanted:
    small_cls_gnn_head_supported with dx), h0, the taps, the bias, the gates and the head. Shapes: small_cls_gnn_head_supported."""
    assert act in _GFL_ACTS, act
    return _small_dense_cell_head(_SmallCellClsGnnHead, ('cls_gnn', head_w, head_b, act, lin_w, lin_b, None), X, h0, wA, wB, bias, graph,
                                  gi, gf)


def small_gates_supported(N, G, F, Kin, Kst, dtype, backward):
    if dtype not in (torch.float32, torch.float64) or os.environ.get('GCRNN_SMALL_GATHER'):
        return False
    return bool(lib.gcrnn_small_gates_supported(dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(backward)))


class _SmallTimeGates(torch.autograd.Function):
    """Both time gates of a small-graph cell for all steps: one launch forward, one backward (reference
    graphML.py:2357-2374). Parameters stacked over (input, forget). Returns gates [2][T][B]. The gradient for X (the gate cells read
    x_t) comes from the backward kernel's dx variant, only when X wants one."""

    @staticmethod
    def forward(ctx, X, h0, wA2, wB2, bias2, lw2, lb2, graph):
        X, h0, wA2, wB2, lw2 = X.contiguous(), h0.contiguous(), wA2.contiguous(), wB2.contiguous(), lw2.contiguous()
        bias2 = bias2.contiguous() if bias2 is not None else None
        lb2 = lb2.contiguous() if lb2 is not None else None
        B, T, G, N = X.shape
        F, Kin, Kst = wA2.shape[1], wA2.shape[2], wB2.shape[2]
        Sd = graph.dense(X.dtype)
        gates = torch.empty((2, T, B), dtype=X.dtype, device=X.device)
        check(lib.gcrnn_small_gates_forward(dtype_code(X.dtype), _p(X), _p(h0), _p(wA2), _p(wB2), _p(bias2), _p(lw2), _p(lb2),
                                            _p(Sd), _p(gates), B, T, N, G, F, Kin, Kst, _stream()), 'small_gates_forward')
        ctx.save_for_backward(X, h0, wA2, wB2, bias2, lw2, gates)
        ctx.graph, ctx.has_lb = graph, lb2 is not None
        return gates

    @staticmethod
    def backward(ctx, dgates):
        X, h0, wA2, wB2, bias2, lw2, gates = ctx.saved_tensors
        B, T, G, N = X.shape
        F, Kin, Kst = wA2.shape[1], wA2.shape[2], wB2.shape[2]
        dt, dev = X.dtype, X.device
        dsum = (dgates * gates * (1 - gates)).contiguous()                    # through the sigmoid
        Sd = ctx.graph.dense(dt)
        pA = torch.empty((B, 2, F, Kin, G), dtype=dt, device=dev)
        pB = torch.empty((B, 2, F, Kst, F), dtype=dt, device=dev)
        pb = torch.empty((B, 2, F), dtype=dt, device=dev)
        plw = torch.empty((B, 2, F * N), dtype=dt, device=dev)
        plb = torch.empty((B, 2), dtype=dt, device=dev)
        pdh0 = torch.empty((B, 2, F, N), dtype=dt, device=dev) if ctx.needs_input_grad[1] else None
        pdX = torch.empty((B, 2, T, G, N), dtype=dt, device=dev) if ctx.needs_input_grad[0] else None
        name = 'small_gates_backward_dx' if pdX is not None else 'small_gates_backward'
        args = (dtype_code(dt), _p(X), _p(h0), _p(wA2), _p(wB2), _p(bias2), _p(lw2), _p(Sd), _p(dsum), _p(pA), _p(pB), _p(pb), _p(plw),
                _p(plb), _p(pdh0))
        check(getattr(lib, 'gcrnn_' + name)(*args, *((_p(pdX),) if pdX is not None else ()), B, T, N, G, F, Kin, Kst, _stream()), name)
        return (pdX[:, 0] + pdX[:, 1] if pdX is not None else None, pdh0.sum(dim=1) if pdh0 is not None else None, pA.sum(dim=0), pB.sum(dim=0),
                pb.sum(dim=0) if bias2 is not None else None, plw.sum(dim=0), plb.sum(dim=0) if ctx.has_lb else None, None)


def small_time_gates(X, h0, wA2, wB2, bias2, lw2, lb2, graph):
    return _SmallTimeGates.apply(X, h0, wA2, wB2, bias2, lw2, lb2, graph)


def small_node_gates_supported(N, G, F, Kin, Kst, dtype, backward):
    """Both node gates of a small-graph cell in one launch (gcrnn_small_node_gates_supported, which implies small_dense_supported with
    gates; GCRNN_SMALL_GATHER=1 answers no, as for small_gates_supported). backward: the backward launch too, with or without dX."""
    if dtype not in (torch.float32, torch.float64) or os.environ.get('GCRNN_SMALL_GATHER'):
        return False
    return bool(lib.gcrnn_small_node_gates_supported(dtype_code(dtype), int(N), int(G), int(F), int(Kin), int(Kst), int(backward)))


class _SmallNodeGates(torch.autograd.Function):
    """Both node gates of a small-graph cell for all steps: one launch forward, one backward (reference graphML.py:2379-2399).
    Parameters stacked over (input, forget); wf2 [2][Kst][F] / bf2 [2] are the F -> 1 graph filters. Returns gates [2][B][T][N]. The
    backward kernel takes the gradient at the pre-sigmoid value, formed here from the saved gates; the gradient for X comes from its dx
    variant, only when X wants one. The per-sequence partial sums are added over B (and the two gates' shares of dX / dh0) by torch's
    deterministic reductions, in a fixed order."""

    @staticmethod
    def forward(ctx, X, h0, wA2, wB2, bias2, wf2, bf2, graph):
        X, h0, wA2, wB2, wf2 = X.contiguous(), h0.contiguous(), wA2.contiguous(), wB2.contiguous(), wf2.contiguous()
        bias2 = bias2.contiguous() if bias2 is not None else None
        bf2 = bf2.contiguous() if bf2 is not None else None
        B, T, G, N = X.shape
        F, Kin, Kst = wA2.shape[1], wA2.shape[2], wB2.shape[2]
        Sd = graph.dense(X.dtype)
        gates = torch.empty((2, B, T, N), dtype=X.dtype, device=X.device)
        check(lib.gcrnn_small_node_gates_forward(dtype_code(X.dtype), _p(X), _p(h0), _p(wA2), _p(wB2), _p(bias2), _p(wf2), _p(bf2),
                                                 _p(Sd), _p(gates), B, T, N, G, F, Kin, Kst, _stream()), 'small_node_gates_forward')
        ctx.save_for_backward(X, h0, wA2, wB2, bias2, wf2, gates)
        ctx.graph, ctx.has_bf = graph, bf2 is not None
        return gates

    @staticmethod
    def backward(ctx, dgates):
        X, h0, wA2, wB2, bias2, wf2, gates = ctx.saved_tensors
        B, T, G, N = X.shape
        F, Kin, Kst = wA2.shape[1], wA2.shape[2], wB2.shape[2]
        dt, dev = X.dtype, X.device
        dl = (dgates * gates * (1 - gates)).contiguous()                      # through the sigmoid
        Sd = ctx.graph.dense(dt)
        pA = torch.empty((B, 2, F, Kin, G), dtype=dt, device=dev)
        pB = torch.empty((B, 2, F, Kst, F), dtype=dt, device=dev)
        pb = torch.empty((B, 2, F), dtype=dt, device=dev)
        pwf = torch.empty((B, 2, Kst, F), dtype=dt, device=dev)
        pbf = torch.empty((B, 2), dtype=dt, device=dev)
        pdh0 = torch.empty((B, 2, F, N), dtype=dt, device=dev) if ctx.needs_input_grad[1] else None
        pdX = torch.empty((B, 2, T, G, N), dtype=dt, device=dev) if ctx.needs_input_grad[0] else None
        name = 'small_node_gates_backward_dx' if pdX is not None else 'small_node_gates_backward'
        args = (dtype_code(dt), _p(X), _p(h0), _p(wA2), _p(wB2), _p(bias2), _p(wf2), _p(Sd), _p(dl), _p(pA), _p(pB), _p(pb), _p(pwf),
                _p(pbf), _p(pdh0))
        check(getattr(lib, 'gcrnn_' + name)(*args, *((_p(pdX),) if pdX is not None else ()), B, T, N, G, F, Kin, Kst, _stream()), name)
        return (pdX[:, 0] + pdX[:, 1] if pdX is not None else None, pdh0.sum(dim=1) if pdh0 is not None else None, pA.sum(dim=0), pB.sum(dim=0),
                pb.sum(dim=0) if bias2 is not None else None, pwf.sum(dim=0), pbf.sum(dim=0) if ctx.has_bf else None, None)


def small_node_gates(X, h0, wA2, wB2, bias2, wf2, bf2, graph):
    """Node gates [2][B][T][N] (input, forget) of a small-graph cell; shapes: small_node_gates_supported."""
    require_device(X, h0, wA2, wB2, wf2)
    return _SmallNodeGates.apply(X, h0, wA2, wB2, bias2, wf2, bf2, graph)


# ------------------------------------------------------------------------------------------ small-graph edge-gated cell
def small_edge_supported(N, nnz, nnz_support, G, F, Kin, Kst, dtype, E=1):
    if E != 1 or dtype not in (torch.float32, torch.float64):
        return False
    return bool(lib.gcrnn_small_edge_supported(dtype_code(dtype), int(N), int(nnz), int(nnz_support), int(G), int(F), int(Kin), int(Kst)))


def _edge_support_values(graph, dtype):
    """(S + I)[m][n] on the attention support in the order of edge_plan()['t_edge'], in the data dtype (the plan itself carries fp32 bits)."""
    cache = graph.__dict__.setdefault('_edge_t_vals', {})
    if dtype not in cache:
        cache[dtype] = graph.mask_vals[0][graph.edge_plan()['t_pos'].long()].to(dtype).contiguous()
    return cache[dtype]


def small_edge_cell_forward(X, h0, wA, wB, bias, graph, att_in, att_f, gi=None, gf=None, last_only=False):
    """Edge-gated cell (optionally time-gated too) on a small graph, inference: the input branch of all steps in one launch, the whole
    recurrence in a second one with one workgroup per sequence. X: B x T x G x N, h0: B x F x N (user layout, fp32 / fp64) -> H: B x T x F x N,
    or B x 1 x F x N (the last state) with last_only. att_in / att_f: (mixer 1 x 1 x 2F, weight 1 x 1 x F x F) of the input / forget
    attention; gi / gf: time gates [T][B] or None."""
    return _small_edge_forward(X, h0, wA, wB, bias, graph, att_in, att_f, gi, gf, last_only)


def _small_edge_forward(X, h0, wA, wB, bias, graph, att_in, att_f, gi, gf, last_only):
    """The two launches of gcrnn_small_edge_forward (inference entry point and the training function's forward)."""
    require_device(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1])
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    dt = X.dtype
    csr = graph.fwd[0]
    plan = graph.edge_plan()
    nnzs = plan['nnz']
    for mixer, weight in (att_in, att_f):
        assert tuple(mixer.shape) == (1, 1, 2 * F) and tuple(weight.shape) == (1, 1, F, F), 'one head, one edge feature, F -> F'
    if not small_edge_supported(N, csr.nnz, nnzs, G, F, Kin, Kst, dt, graph.E):
        raise GcrnnError('small_edge_cell_forward: shape outside the one-launch edge-gated kernel (small_edge_supported)')
    H = torch.empty((B, 1 if last_only else T, F, N), dtype=dt, device=X.device)
    Ya = torch.empty((B, T, F, N), dtype=dt, device=X.device)         # the first launch's output, the second one's input; not kept
    bvec = bias.detach().contiguous().view(-1) if bias is not None else None
    if gi is not None:
        assert tuple(gi.shape) == (T, B) and tuple(gf.shape) == (T, B)
        gi, gf = gi.detach().to(dt).contiguous(), gf.detach().to(dt).contiguous()
    ops_in = [t.detach().contiguous() for t in (X, h0, wA, wB)]
    atts = [t.detach().contiguous() for t in (att_in[1], att_in[0], att_f[1], att_f[0])]
    assert all(t.dtype == dt for t in ops_in + atts) and (bvec is None or bvec.dtype == dt)
    vals, tvals = csr.val(dt), _edge_support_values(graph, dt)
    check(lib.gcrnn_small_edge_forward(dtype_code(dt), _p(ops_in[0]), _p(ops_in[1]), _p(ops_in[2]), _p(ops_in[3]), _p(bvec),
                                       _p(atts[0]), _p(atts[1]), _p(atts[2]), _p(atts[3]), _p(gi), _p(gf),
                                       _p(csr.rowptr), _p(csr.col), _p(vals), _p(plan['rowptr']), _p(plan['r_edge']),
                                       _p(plan['t_rowptr']), _p(plan['t_edge']), _p(tvals), _p(Ya), _p(H),
                                       B, T, N, G, F, Kin, Kst, csr.nnz, nnzs, int(bool(last_only)), _stream()), 'small_edge_forward')
    return H


def small_edge_training_supported(N, nnz, nnz_support, G, F, Kin, Kst, dtype, E=1):
    if E != 1 or dtype not in (torch.float32, torch.float64):
        return False
    return bool(lib.gcrnn_small_edge_backward_supported(dtype_code(dtype), int(N), int(nnz), int(nnz_support), int(G), int(F),
                                                        int(Kin), int(Kst)))


def small_edge_input_grad_supported(N, nnz, nnz_support, G, F, Kin, Kst, dtype, E=1):
    """The edge-gated BPTT also returns dX: the same answer as small_edge_training_supported (the backward kernels' LDS image is sized for
    max(G, F) channels in both launches, so the input branch's hop adjoint adds nothing). The counterpart of small_input_grad_supported."""
    return small_edge_training_supported(N, nnz, nnz_support, G, F, Kin, Kst, dtype, E)


def _edge_unfold(pwf, pbf, w, bias, mixer, weight):
    """Gradients of one branch's taps w [F][1][K][C], bias, attention mixer and weight from the per-workgroup gradients of the folded
    taps wf = [W w ; a1^T W w ; a2^T W w] (pwf [slots][F+2][K][C]) and of the folded bias (pbf [slots][F+2])."""
    F = w.shape[0]
    dwf, dbf = pwf.sum(dim=0).view(F + 2, -1), pbf.sum(dim=0)
    w2, W, a = w.reshape(F, -1), weight.view(F, F), mixer.view(2, F)
    top = dwf[:F] + a.t() @ dwf[F:]                                  # d loss / d (W w)
    topb = dbf[:F] + a.t() @ dbf[F:]                                 # d loss / d (W b)
    da = dwf[F:] @ (W @ w2).t()
    dW = top @ w2.t()
    db = None
    if bias is not None:
        bv = bias.view(F)
        da = da + dbf[F:].unsqueeze(1) * (W @ bv).unsqueeze(0)
        dW = dW + topb.unsqueeze(1) * bv.unsqueeze(0)
        db = (W.t() @ topb).view(F, 1)
    return (W.t() @ top).view(w.shape), db, da.reshape(mixer.shape), dW.view(weight.shape)


class _SmallEdgeCell(torch.autograd.Function):
    """Edge-gated small-graph cell with BPTT: forward = the two launches of the inference path (all states kept), backward = two launches
    (small_edge_bptt_kernel, recurrence then input branch) plus the unfolding of the folded taps' gradients. Gradients for h0, the taps, the
    bias, both attentions' mixer and weight and the time gates; for X too when it wants one (the input-branch launch's dx variant, which
    goes on to the hops' adjoint; no launch is added)."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H = _small_edge_forward(X, h0, wA, wB, bias, graph, (m_in, w_in), (m_f, w_f), gi, gf, False)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf)
        ctx.graph = graph
        return H

    @staticmethod
    def backward(ctx, dH):
        X, h0, H, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf = ctx.saved_tensors
        B, T, G, N = X.shape
        F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
        dt, dev = X.dtype, X.device
        graph = ctx.graph
        fwd, adj, plan = graph.fwd[0], graph.adj[0], graph.edge_plan()
        nnzs = plan['nnz']
        R = F + 2
        dPre = torch.empty((B, T, F, N), dtype=dt, device=dev)
        pwfA = torch.empty((B * T, R, Kin, G), dtype=dt, device=dev)
        pbfA = torch.empty((B * T, R), dtype=dt, device=dev)
        pwfB = torch.empty((B, R, Kst, F), dtype=dt, device=dev)
        pbfB = torch.empty((B, R), dtype=dt, device=dev)
        dgi = dgf = None
        if gi is not None:
            gi, gf = gi.to(dt).contiguous(), gf.to(dt).contiguous()
            dgi = torch.empty((T, B), dtype=dt, device=dev)
            dgf = torch.empty((T, B), dtype=dt, device=dev)
        dh0 = torch.empty_like(h0) if ctx.needs_input_grad[1] else None
        dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
        bvec = bias.contiguous().view(-1) if bias is not None else None
        # every operand is a named local (see _small_dense_bptt)
        dHc, wAc, wBc = dH.contiguous(), wA.contiguous(), wB.contiguous()
        wi, ai, wfo, afo = w_in.contiguous(), m_in.contiguous(), w_f.contiguous(), m_f.contiguous()
        fval, aval, tvals = fwd.val(dt), adj.val(dt), _edge_support_values(graph, dt)
        name = 'small_edge_backward_dx' if dX is not None else 'small_edge_backward'
        args = (dtype_code(dt), _p(X), _p(h0), _p(H), _p(dHc), _p(wAc), _p(wBc), _p(bvec), _p(wi), _p(ai), _p(wfo), _p(afo), _p(gi), _p(gf),
                _p(fwd.rowptr), _p(fwd.col), _p(fval), _p(adj.rowptr), _p(adj.col), _p(aval),
                _p(plan['rowptr']), _p(plan['r_edge']), _p(plan['t_rowptr']), _p(plan['t_edge']), _p(tvals), _p(plan['t_pos']),
                _p(dPre), _p(pwfA), _p(pbfA), _p(pwfB), _p(pbfB), _p(dgi), _p(dgf), _p(dh0))
        check(getattr(lib, 'gcrnn_' + name)(*args, *((_p(dX),) if dX is not None else ()), B, T, N, G, F, Kin, Kst, fwd.nnz, nnzs, _stream()),
              name)
        dwA, dbA, dm_in, dw_in = _edge_unfold(pwfA, pbfA, wAc, bias, ai, wi)
        dwB, dbB, dm_f, dw_f = _edge_unfold(pwfB, pbfB, wBc, bias, afo, wfo)
        db = dbA + dbB if bias is not None else None              # one bias, both branches
        return dX, dh0, dwA, dwB, db, dm_in, dw_in, dm_f, dw_f, dgi, dgf, None


def small_edge_cell_train(X, h0, wA, wB, bias, graph, att_in, att_f, gi=None, gf=None):
    """Training forward of the edge-gated small-graph cell (small_edge_training_supported shapes). att_in / att_f: (mixer, weight) of the
    input / forget attention; gi / gf: differentiable time gates [T][B] or None. Gradients for everything that wants one, X included
    (small_edge_input_grad_supported: the same shapes); an X without requires_grad costs nothing extra."""
    require_device(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1])
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    if not small_edge_training_supported(N, graph.fwd[0].nnz, graph.edge_plan()['nnz'], G, F, Kin, Kst, X.dtype, graph.E):
        raise GcrnnError('small_edge_cell_train: shape outside the edge-gated BPTT kernel (small_edge_training_supported)')
    return _SmallEdgeCell.apply(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], gi, gf, graph)


# ---- the edge-gated models on small graphs: the read-out on the last state / the per-node head inside the recurrence launches
SMALL_EDGE_HEAD_LAST, SMALL_EDGE_HEAD_NODE = 1, 2                     # gcrnn.h: GCRNN_SMALL_EDGE_HEAD_*


def small_edge_head_supported(N, nnz, nnz_support, G, F, Kin, Kst, head_kind, NC, dtype, backward, E=1):
    """The one-launch edge-gated kernels take this cell with a head inside the recurrence launches (gcrnn_small_edge_head_supported):
    head_kind SMALL_EDGE_HEAD_LAST, NC classes read out of the last state, or SMALL_EDGE_HEAD_NODE, NC <= 8 outputs per node on every
    state. backward: the training step (never more than small_edge_training_supported admits)."""
    if E != 1 or dtype not in (torch.float32, torch.float64):
        return False
    return bool(lib.gcrnn_small_edge_head_supported(dtype_code(dtype), int(N), int(nnz), int(nnz_support), int(G), int(F), int(Kin),
                                                    int(Kst), int(head_kind), int(NC), int(bool(backward))))


def _small_edge_forward_head(X, h0, wA, wB, bias, graph, att_in, att_f, gi, gf, head_kind, head_w, head_b, store):
    """The two launches of gcrnn_small_edge_forward_head: (H or None, logits [B][NC] / Y [B][T][NC][N]). Every operand is a named local up
    to the launch (_small_dense_bptt)."""
    require_device(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], head_w, head_b)
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    dt, dev = X.dtype, X.device
    csr = graph.fwd[0]
    plan = graph.edge_plan()
    nnzs = plan['nnz']
    NC = head_w.shape[0]
    for mixer, weight in (att_in, att_f):
        assert tuple(mixer.shape) == (1, 1, 2 * F) and tuple(weight.shape) == (1, 1, F, F), 'one head, one edge feature, F -> F'
    assert tuple(head_w.shape) == ((NC, F * N) if head_kind == SMALL_EDGE_HEAD_LAST else (NC, F)) and head_w.dtype == dt
    assert head_b is None or (head_b.dtype == dt and head_b.numel() == NC)
    if not small_edge_head_supported(N, csr.nnz, nnzs, G, F, Kin, Kst, head_kind, NC, dt, False, graph.E):
        raise GcrnnError('small_edge head: shape outside the one-launch edge-gated kernel with a head (small_edge_head_supported)')
    H = None if store == SMALL_STATES_NONE else torch.empty((B, T if store == SMALL_STATES_ALL else 1, F, N), dtype=dt, device=dev)
    Ya = torch.empty((B, T, F, N), dtype=dt, device=dev)              # the first launch's output, the second one's input; not kept
    out = torch.empty((B, NC) if head_kind == SMALL_EDGE_HEAD_LAST else (B, T, NC, N), dtype=dt, device=dev)
    bvec = bias.detach().contiguous().view(-1) if bias is not None else None
    if gi is not None:
        assert tuple(gi.shape) == (T, B) and tuple(gf.shape) == (T, B)
        gi, gf = gi.detach().to(dt).contiguous(), gf.detach().to(dt).contiguous()
    Xc, h0c, wAc, wBc = X.detach().contiguous(), h0.detach().contiguous(), wA.detach().contiguous(), wB.detach().contiguous()
    wi, ai, wfo, afo = [t.detach().contiguous() for t in (att_in[1], att_in[0], att_f[1], att_f[0])]
    hw = head_w.detach().contiguous()
    hb = head_b.detach().contiguous() if head_b is not None else None
    assert all(t.dtype == dt for t in (Xc, h0c, wAc, wBc, wi, ai, wfo, afo)) and (bvec is None or bvec.dtype == dt)
    vals, tvals = csr.val(dt), _edge_support_values(graph, dt)
    check(lib.gcrnn_small_edge_forward_head(dtype_code(dt), _p(Xc), _p(h0c), _p(wAc), _p(wBc), _p(bvec), _p(wi), _p(ai), _p(wfo), _p(afo),
                                            _p(gi), _p(gf), _p(csr.rowptr), _p(csr.col), _p(vals), _p(plan['rowptr']), _p(plan['r_edge']),
                                            _p(plan['t_rowptr']), _p(plan['t_edge']), _p(tvals), _p(Ya), _p(H), _p(hw), _p(hb), _p(out),
                                            B, T, N, G, F, Kin, Kst, csr.nnz, nnzs, NC, head_kind, store, _stream()),
          'small_edge_forward_head')
    return H, out


def _small_edge_bptt_head(ctx, head_kind, up, head_w):
    """The two BPTT launches of gcrnn_small_edge_backward_head from what the forward saved, and the unfolding of the folded taps'
    gradients: the gradients of _SmallEdgeCell.backward (dX .. dgf). up: dlogits [B][NC] or dY [B][T][NC][N], contiguous."""
    X, h0, H, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf = ctx.saved_tensors[:12]
    B, T, G, N = X.shape
    F, Kin, Kst = wA.shape[0], wA.shape[2], wB.shape[2]
    dt, dev = X.dtype, X.device
    graph = ctx.graph
    fwd, adj, plan = graph.fwd[0], graph.adj[0], graph.edge_plan()
    nnzs = plan['nnz']
    NC = head_w.shape[0]
    if not small_edge_head_supported(N, fwd.nnz, nnzs, G, F, Kin, Kst, head_kind, NC, dt, True, graph.E):
        raise GcrnnError('small_edge head: shape outside the edge-gated BPTT kernel with a head (small_edge_head_supported, backward)')
    R = F + 2
    dPre = torch.empty((B, T, F, N), dtype=dt, device=dev)
    pwfA = torch.empty((B * T, R, Kin, G), dtype=dt, device=dev)
    pbfA = torch.empty((B * T, R), dtype=dt, device=dev)
    pwfB = torch.empty((B, R, Kst, F), dtype=dt, device=dev)
    pbfB = torch.empty((B, R), dtype=dt, device=dev)
    dgi = dgf = None
    if gi is not None:
        gi, gf = gi.to(dt).contiguous(), gf.to(dt).contiguous()
        dgi = torch.empty((T, B), dtype=dt, device=dev)
        dgf = torch.empty((T, B), dtype=dt, device=dev)
    dh0 = torch.empty_like(h0) if ctx.needs_input_grad[1] else None
    dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
    bvec = bias.contiguous().view(-1) if bias is not None else None
    assert up.is_contiguous() and head_w.is_contiguous()
    wAc, wBc = wA.contiguous(), wB.contiguous()
    wi, ai, wfo, afo = w_in.contiguous(), m_in.contiguous(), w_f.contiguous(), m_f.contiguous()
    fval, aval, tvals = fwd.val(dt), adj.val(dt), _edge_support_values(graph, dt)
    check(lib.gcrnn_small_edge_backward_head(dtype_code(dt), _p(X), _p(h0), _p(H), _p(up), _p(head_w), _p(wAc), _p(wBc), _p(bvec), _p(wi),
                                             _p(ai), _p(wfo), _p(afo), _p(gi), _p(gf), _p(fwd.rowptr), _p(fwd.col), _p(fval),
                                             _p(adj.rowptr), _p(adj.col), _p(aval), _p(plan['rowptr']), _p(plan['r_edge']),
                                             _p(plan['t_rowptr']), _p(plan['t_edge']), _p(tvals), _p(plan['t_pos']), _p(dPre), _p(pwfA),
                                             _p(pbfA), _p(pwfB), _p(pbfB), _p(dgi), _p(dgf), _p(dh0), _p(dX), B, T, N, G, F, Kin, Kst,
                                             fwd.nnz, nnzs, NC, head_kind, _stream()), 'small_edge_backward_head')
    dwA, dbA, dm_in, dw_in = _edge_unfold(pwfA, pbfA, wAc, bias, ai, wi)
    dwB, dbB, dm_f, dw_f = _edge_unfold(pwfB, pbfB, wBc, bias, afo, wfo)
    db = dbA + dbB if bias is not None else None                  # one bias, both branches
    return dX, dh0, dwA, dwB, db, dm_in, dw_in, dm_f, dw_f, dgi, dgf


class _SmallEdgeCellHead(torch.autograd.Function):
    """Edge-gated small-graph cell + Linear(F N -> C) on its last state as ONE autograd node. Forward: the two launches, every state kept
    (BPTT reads them), the logits from the recurrence launch. Backward: the two BPTT launches, the recurrence seeded from dlogits inside
    the kernel (gcrnn_small_edge_backward_head: no dH [B][T][F][N] is allocated, zero-filled or read), plus the library product for the
    head's own parameters."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf, head_w, head_b, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H, logits = _small_edge_forward_head(X, h0, wA, wB, bias, graph, (m_in, w_in), (m_f, w_f), gi, gf, SMALL_EDGE_HEAD_LAST, head_w,
                                             head_b, SMALL_STATES_ALL)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf, head_w)
        ctx.graph, ctx.has_hb = graph, head_b is not None
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        H, head_w = ctx.saved_tensors[2], ctx.saved_tensors[12]
        dlc, hw = dlogits.contiguous(), head_w.detach().contiguous()
        grads = _small_edge_bptt_head(ctx, SMALL_EDGE_HEAD_LAST, dlc, hw)
        return grads + _readout_grads(dlc, H[:, -1], ctx.needs_input_grad[11], ctx.has_hb and ctx.needs_input_grad[12]) + (None,)


class _SmallEdgeCellNodeHead(torch.autograd.Function):
    """Edge-gated small-graph cell + Linear(F -> O) shared by all nodes on every state as ONE autograd node. Forward: the two launches,
    every state kept, Y from the recurrence launch. Backward: the two BPTT launches, the recurrence forming dH_t = node_w^T dY_t inside the
    kernel (gcrnn_small_edge_backward_head: no dH [B][T][F][N] is allocated, written or read), plus the head's own gradients as
    _SmallCellNodeHead makes them."""

    @staticmethod
    def forward(ctx, X, h0, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf, node_w, node_b, graph):
        X, h0 = X.contiguous(), h0.contiguous()
        H, Y = _small_edge_forward_head(X, h0, wA, wB, bias, graph, (m_in, w_in), (m_f, w_f), gi, gf, SMALL_EDGE_HEAD_NODE, node_w, node_b,
                                        SMALL_STATES_ALL)
        ctx.save_for_backward(X, h0, H, wA, wB, bias, m_in, w_in, m_f, w_f, gi, gf, node_w)
        ctx.graph, ctx.has_nb = graph, node_b is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        H, node_w = ctx.saved_tensors[2], ctx.saved_tensors[12]
        B, T, F, N = H.shape
        O = node_w.shape[0]
        dYc, nw = dY.contiguous(), node_w.detach().contiguous()
        grads = _small_edge_bptt_head(ctx, SMALL_EDGE_HEAD_NODE, dYc, nw)
        return grads + _node_head_grads(H.view(B * T, F, N), dYc.view(B * T, O, N), nw, ctx.needs_input_grad[11],
                                        ctx.has_nb and ctx.needs_input_grad[12], bias_kernel=False, bias_level0=False) + (None,)


def _small_edge_cell_head(fn, head_kind, X, h0, wA, wB, bias, graph, att_in, att_f, head_w, head_b, gi, gf):
    require_device(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], head_w)
    if not _wants_grad(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], gi, gf, head_w, head_b):
        return _small_edge_forward_head(X, h0, wA, wB, bias, graph, att_in, att_f, gi, gf, head_kind, head_w, head_b, SMALL_STATES_NONE)[1]
    return fn.apply(X, h0, wA, wB, bias, att_in[0], att_in[1], att_f[0], att_f[1], gi, gf, head_w, head_b, graph)


def small_edge_cell_classify(X, h0, wA, wB, bias, graph, att_in, att_f, head_w, head_b, gi=None, gf=None):
    """The edge-gated small-graph cell followed by Linear(F N -> C) on its last state (head_w [C][F*N], head_b [C] or None, the states'
    dtype): logits [B][C]. att_in / att_f: (mixer, weight) of the input / forget attention; gi / gf: time gates [T][B] or None. Where
    nothing wants a gradient it is one forward call that stores no state; otherwise one autograd node (_SmallEdgeCellHead) with gradients
    for everything that wants one, X included. Shapes: small_edge_head_supported."""
    return _small_edge_cell_head(_SmallEdgeCellHead, SMALL_EDGE_HEAD_LAST, X, h0, wA, wB, bias, graph, att_in, att_f, head_w, head_b, gi, gf)


def small_edge_cell_regress(X, h0, wA, wB, bias, graph, att_in, att_f, node_w, node_b, gi=None, gf=None):
    """The edge-gated small-graph cell followed by Linear(F -> O) shared by all nodes on every state (node_w [O][F], node_b [O] or None,
    the states' dtype): Y [B][T][O][N]. Otherwise as small_edge_cell_classify (_SmallEdgeCellNodeHead). Shapes: small_edge_head_supported."""
    return _small_edge_cell_head(_SmallEdgeCellNodeHead, SMALL_EDGE_HEAD_NODE, X, h0, wA, wB, bias, graph, att_in, att_f, node_w, node_b,
                                 gi, gf)


# ------------------------------------------------------------------------------------------ per-node head
def node_linear_supported(F, O, dtype, N=None, wdtype=None):
    if dtype == torch.bfloat16:            # bf16 activations (the fused cell's output), fp32 master or bf16 parameters
        return N is not None and wdtype in (torch.float32, torch.bfloat16) and \
            bool(lib.gcrnn_node_linear_bf16_supported(int(N), int(F), int(O)))
    return dtype in (torch.float32, torch.float64) and (wdtype is None or wdtype == dtype) and 0 < F <= 64 and 0 < O <= 8


class _NodeLinear(torch.autograd.Function):
    """y[r][o][n] = sum_f w[o][f] h[r][f][n] + b[o] on the user layout (the 'multipMlp' head, architectures.py:1616-1627).
    fp32 / fp64 throughout, or bf16 activations with fp32 / bf16 parameters (fp32 accumulation, bf16 output)."""

    @staticmethod
    def forward(ctx, h, w, b):
        require_device(h, w)
        hc, wc = h.contiguous(), w.contiguous()
        bc = b.contiguous() if b is not None else None
        R, F, N = hc.shape
        O = wc.shape[0]
        y = torch.empty((R, O, N), dtype=hc.dtype, device=hc.device)
        if hc.dtype == torch.bfloat16:
            assert bc is None or bc.dtype == wc.dtype
            check(lib.gcrnn_node_linear_bf16_forward(dtype_code(wc.dtype), _p(hc), _p(wc), _p(bc), _p(y), R, N, F, O, _stream()),
                  'node_linear_bf16_forward')
        else:
            check(lib.gcrnn_node_linear_forward(dtype_code(hc.dtype), _p(hc), _p(wc), _p(bc), _p(y), R, N, F, O, _stream()),
                  'node_linear_forward')
        ctx.save_for_backward(hc, wc)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        h, w = ctx.saved_tensors
        R, F, N = h.shape
        O = w.shape[0]
        dyc = dy.contiguous()
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        if h.dtype == torch.bfloat16:
            dyc = dyc.to(torch.bfloat16)
            nb = int(lib.gcrnn_node_linear_bf16_blocks(R, N))
            pw = torch.empty((nb, O, F), dtype=torch.float32, device=h.device)
            pb = torch.empty((nb, O), dtype=torch.float32, device=h.device)
            check(lib.gcrnn_node_linear_bf16_backward(dtype_code(w.dtype), _p(h), _p(w), _p(dyc), _p(dh), _p(pw), _p(pb), R, N, F, O,
                                                      _stream()), 'node_linear_bf16_backward')
            return dh, pw.sum(dim=0).to(w.dtype), (pb.sum(dim=0).to(w.dtype) if ctx.has_bias else None)
        nb = int(lib.gcrnn_node_linear_blocks(R, N))
        pw = torch.empty((nb, O, F), dtype=h.dtype, device=h.device)
        pb = torch.empty((nb, O), dtype=h.dtype, device=h.device)
        check(lib.gcrnn_node_linear_backward(dtype_code(h.dtype), _p(h), _p(w), _p(dyc), _p(dh), _p(pw), _p(pb), R, N, F, O,
                                             _stream()), 'node_linear_backward')
        return dh, pw.sum(dim=0), (pb.sum(dim=0) if ctx.has_bias else None)


def node_linear(h, weight, bias=None):
    return _NodeLinear.apply(h, weight, bias)


# ------------------------------------------------------------------------------------------ graph-filter layer (GNN output heads)
_GFL_ACTS = {None: 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3}


def _gfl_uniform(csr):
    """The one weight every edge of `csr` carries (0.0: weights differ). Read once per CSR and kept on it."""
    u = getattr(csr, '_gfl_uniform', None)
    if u is None:
        v = csr.val(torch.float64)
        u = float(v[0]) if csr.nnz > 0 and bool((v == v[0]).all()) else 0.0
        csr._gfl_uniform = u
    return u


def graph_filter_layer_supported(x_dtype, w_dtype, graph, F_in, F_out, K):
    """True when gcrnn_graph_filter_layer_{forward,backward} evaluate this layer: bf16 x with fp32 parameters, or fp32 / fp64
    throughout; E = 1, N <= 1024 and an LDS image that fits one CU."""
    if not ((x_dtype == torch.bfloat16 and w_dtype == torch.float32) or (x_dtype == w_dtype and x_dtype in (torch.float32, torch.float64))):
        return False
    if graph.E != 1:
        return False
    csr = graph.fwd[0]
    uni = int(_gfl_uniform(csr) != 0.0 and _gfl_uniform(graph.adj[0]) != 0.0)
    return bool(lib.gcrnn_graph_filter_layer_supported(dtype_code(x_dtype), graph.N, csr.nnz, graph.E, int(F_in), int(F_out), int(K), uni))


class _GraphFilterLayer(torch.autograd.Function):
    """act(LSIGF(w, S, x, b)) of one GraphFilter (graphML.py:1086-1205) in one launch per pass (gcrnn_readout.hip).
    x [items][F_in][N] -> y [items][F_out][N] in the parameters' dtype; the parameters are read as they are on every call."""

    @staticmethod
    def forward(ctx, x, w, b, graph, act):
        require_device(x, w, b)
        xc, wc = x.contiguous(), w.contiguous()
        bc = b.contiguous() if b is not None else None
        items, Fin, N = xc.shape
        Fout, E, K, _ = wc.shape
        csr = graph.fwd[0]
        uw = _gfl_uniform(csr)
        y = torch.empty((items, Fout, N), dtype=wc.dtype, device=xc.device)
        check(lib.gcrnn_graph_filter_layer_forward(dtype_code(xc.dtype), _p(xc), _p(wc), _p(bc), _p(y), _p(csr.rowptr), _p(csr.col),
                                                   None if uw else _p(csr.val(wc.dtype)), uw, items, N, csr.nnz, E, Fin, Fout, K,
                                                   _GFL_ACTS[act], _stream()), 'graph_filter_layer_forward')
        ctx.save_for_backward(xc, wc, y)
        ctx.graph, ctx.act, ctx.has_bias = graph, act, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        items, Fin, N = x.shape
        Fout, E, K, _ = w.shape
        adj = ctx.graph.adj[0]
        uw = _gfl_uniform(adj)
        code = dtype_code(x.dtype)
        slots = int(lib.gcrnn_graph_filter_layer_wgrad_slots(code, items, N, adj.nnz, Fin, Fout, K, int(uw != 0.0)))
        dwp = torch.empty((slots, Fout * K * Fin), dtype=w.dtype, device=x.device)
        dbp = torch.empty((slots, Fout), dtype=w.dtype, device=x.device) if ctx.has_bias else None
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dyc = dy.contiguous().to(w.dtype)
        check(lib.gcrnn_graph_filter_layer_backward(code, _p(x), _p(w), _p(y), _p(dyc), _p(dx), _p(dwp), _p(dbp), slots, _p(adj.rowptr),
                                                    _p(adj.col), None if uw else _p(adj.val(w.dtype)), uw, items, N, adj.nnz, E, Fin,
                                                    Fout, K, _GFL_ACTS[ctx.act], _stream()), 'graph_filter_layer_backward')
        dw = dwp.sum(dim=0).reshape(w.shape)
        db = dbp.sum(dim=0).reshape(Fout, 1) if ctx.has_bias else None
        return dx, dw, db, None, None


def _graph_filter_layer_composed(x, weight, bias, graph, act):
    """The composed path outside the kernel's envelope: GraphFilter.forward (LSIGF on the node-major filter ops) + the torch
    activation, in the parameters' dtype."""
    from .Utils import graphML as gml
    y = gml.LSIGF(weight, graph, x.to(weight.dtype), bias)
    return {None: lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[act](y)


def graph_filter_layer(x, weight, bias, graph, act=None):
    """y = act( sum_k w[:, 0, k, :] (x S^k) + b ) for x [items][F_in][N], weight F_out x E x K x F_in, bias F_out x 1 (or None),
    act in (None, 'relu', 'tanh', 'sigmoid'). One HIP launch per pass where graph_filter_layer_supported says so, else the composed
    filter path."""
    assert act in _GFL_ACTS, act
    assert x.dim() == 3 and x.shape[1] == weight.shape[3] and x.shape[2] == graph.N, (tuple(x.shape), tuple(weight.shape), graph.N)
    Fout, E, K, Fin = weight.shape
    if graph.device != x.device:
        graph = graph.to(x.device)
    if x.is_cuda and E == graph.E and graph_filter_layer_supported(x.dtype, weight.dtype, graph, Fin, Fout, K) and \
            (bias is None or bias.dtype == weight.dtype):
        return _GraphFilterLayer.apply(x, weight, bias, graph, act)
    return _graph_filter_layer_composed(x, weight, bias, graph, act)


# ------------------------------------------------------------------------------------------ plain RNN (the drivers' RNN baselines)
_RNN_ACTS = {'tanh': 0, 'relu': 1}


def rnn_supported(dtype, B, T, D, F_h):
    """True when gcrnn_rnn_{forward,backward} evaluate this recurrence: fp32 or fp64, 1 <= F_h <= 64, D <= 65536 (gcrnn_rnn.h)."""
    if dtype not in (torch.float32, torch.float64):
        return False
    return bool(lib.gcrnn_rnn_supported(dtype_code(dtype), int(B), int(T), int(D), int(F_h)))


class _RnnSequence(torch.autograd.Function):
    """H = torch.nn.RNN(D, F_h, 1, nonlinearity, bias, batch_first=True)(x, h0)[0] on the HIP kernels (gcrnn_rnn.hip): two launches
    forward, at most three backward plus the sum of the weight-gradient slots, whatever T is."""

    @staticmethod
    def forward(ctx, x, h0, w_ih, w_hh, b_ih, b_hh, nonlinearity):
        require_device(x, h0, w_ih, w_hh, b_ih, b_hh)
        xc, hc, wi, wh = x.contiguous(), h0.contiguous(), w_ih.contiguous(), w_hh.contiguous()
        bi = b_ih.contiguous() if b_ih is not None else None
        bh = b_hh.contiguous() if b_hh is not None else None
        B, T, D = xc.shape
        Fh = wh.shape[0]
        H = torch.empty((B, T, Fh), dtype=xc.dtype, device=xc.device)
        check(lib.gcrnn_rnn_forward(dtype_code(xc.dtype), _p(xc), _p(hc), _p(wi), _p(wh), _p(bi), _p(bh), _p(H), B, T, D, Fh,
                                    _RNN_ACTS[nonlinearity], _stream()), 'rnn_forward')
        ctx.save_for_backward(xc, hc, wi, wh, H)
        ctx.act, ctx.has_bias = _RNN_ACTS[nonlinearity], b_ih is not None
        return H

    @staticmethod
    def backward(ctx, dH):
        x, h0, wi, wh, H = ctx.saved_tensors
        B, T, D = x.shape
        Fh = wh.shape[0]
        code = dtype_code(x.dtype)
        slots = int(lib.gcrnn_rnn_wgrad_slots(code, B, T, D, Fh))
        parts = torch.empty((slots, Fh, D + Fh + 1), dtype=x.dtype, device=x.device)
        dZ = torch.empty_like(H)
        dh0 = torch.empty_like(h0) if ctx.needs_input_grad[1] else None
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dHc = dH.contiguous().to(x.dtype)
        check(lib.gcrnn_rnn_backward(code, _p(x), _p(h0), _p(wi), _p(wh), _p(H), _p(dHc), _p(dZ), _p(dh0), _p(dx), _p(parts), slots,
                                     B, T, D, Fh, ctx.act, _stream()), 'rnn_backward')
        dw = parts.sum(dim=0)
        dwi, dwh = dw[:, :D], dw[:, D:D + Fh]
        db = dw[:, D + Fh] if ctx.has_bias else None
        return dx, dh0, dwi, dwh, db, (db.clone() if db is not None else None), None


def _rnn_sequence_composed(x, h0, w_ih, w_hh, b_ih, b_hh, nonlinearity):
    """The composed path outside the kernels' envelope: torch matmul + the activation, step by step, under autograd."""
    act = torch.tanh if nonlinearity == 'tanh' else torch.relu
    U = x.matmul(w_ih.t())
    if b_ih is not None:
        U = U + (b_ih + b_hh)
    h, hs = h0, []
    for t in range(x.shape[1]):
        h = act(U[:, t] + h.matmul(w_hh.t()))
        hs.append(h)
    return torch.stack(hs, dim=1)


def rnn_sequence(x, h0, w_ih, w_hh, b_ih, b_hh, nonlinearity):
    """H [B][T][F_h] of h_t = act(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh) for x [B][T][D], h0 [B][F_h], w_ih F_h x D, w_hh F_h x F_h,
    b_ih / b_hh F_h (or both None), nonlinearity 'tanh' or 'relu'. x is computed in the parameters' dtype (bf16 activations with
    fp32 parameters). The HIP kernels where rnn_supported says so, else the composed step-by-step path. CPU tensors raise."""
    if nonlinearity not in _RNN_ACTS:
        raise ValueError("Unknown nonlinearity '%s'. Select from 'tanh' or 'relu'." % (nonlinearity,))
    assert (b_ih is None) == (b_hh is None)
    require_device(x, h0, w_ih, w_hh, b_ih, b_hh)
    assert x.dim() == 3 and h0.dim() == 2 and x.shape[2] == w_ih.shape[1] and h0.shape == (x.shape[0], w_hh.shape[0]), \
        (tuple(x.shape), tuple(h0.shape), tuple(w_ih.shape), tuple(w_hh.shape))
    x, h0 = x.to(w_ih.dtype), h0.to(w_ih.dtype)
    B, T, D = x.shape
    if rnn_supported(w_ih.dtype, B, T, D, w_hh.shape[0]):
        return _RnnSequence.apply(x, h0, w_ih, w_hh, b_ih, b_hh, nonlinearity)
    return _rnn_sequence_composed(x, h0, w_ih, w_hh, b_ih, b_hh, nonlinearity)


# ------------------------------------------------------------------------------------------ loss
class _L1Loss(torch.autograd.Function):
    """mean |x - y| with the gradient produced in the same pass (reference batchTimeL1Loss, miscTools.py:112-119)."""

    @staticmethod
    def forward(ctx, x, y):
        require_device(x, y)
        xc, yc = x.contiguous(), y.contiguous()
        if xc.data_ptr() % 16:                       # the kernel moves 16-byte vectors: re-base a slice with an odd offset
            xc = xc.clone()
        if yc.data_ptr() % 16:
            yc = yc.clone()
        n = xc.numel()
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        grad = torch.empty_like(xc) if want else None
        acc_dt = torch.float64 if xc.dtype == torch.float64 else torch.float32
        partial = torch.empty((int(lib.gcrnn_l1_loss_blocks(n)),), dtype=acc_dt, device=xc.device)
        check(lib.gcrnn_l1_loss(dtype_code(xc.dtype), _p(xc), _p(yc), _p(grad), _p(partial), n, 1.0 / n, _stream()), 'l1_loss')
        ctx.grad = grad
        ctx.used = False
        ctx.operands = (xc, yc) if want else None      # (references, no copies: a second backward recomputes the gradient from them)
        return (partial.sum() / n).to(x.dtype)

    @staticmethod
    def backward(ctx, gout):
        g = ctx.grad
        if g is not None:
            if ctx.used:
                # the buffer was scaled in place and handed out by the first backward (other tensors may alias it): a second backward over a
                # retained graph (several heads, gradient-penalty loops -- torch's own L1Loss allows it, miscTools.py:112-119) gets a FRESH
                # tensor recomputed from the operands, sign(x - y) * gout / n, instead
                xc, yc = ctx.operands
                g2 = torch.sign(xc - yc) * (gout.detach().to(xc.dtype) / xc.numel())
                return (g2 if ctx.needs_input_grad[0] else None), (-g2 if ctx.needs_input_grad[1] else None)
            ctx.used = True
            # chain rule through the scalar loss WITHOUT a pass over g when the upstream gradient is 1 (loss.backward()): the kernel
            # reads the device scalar r = gout and returns at once when r == 1 (no host sync: capturable)
            r = gout.detach().to(torch.float64 if g.dtype == torch.float64 else torch.float32).reshape(1).contiguous()
            check(lib.gcrnn_scale_unless_one(dtype_code(g.dtype), _p(g), _p(r), g.numel(), _stream()), 'scale_unless_one')
        return (g if ctx.needs_input_grad[0] else None), (-g if (g is not None and ctx.needs_input_grad[1]) else None)


def l1_loss(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    return _L1Loss.apply(x, y)


def batch_time_mse(xv, yv):
    """mean_c sqrt(sum_r (x - y)^2) / sqrt(sum_r y^2) of two [R][C] matrices (reference batchTimeMSELoss,
    miscTools.py:121-130); no autograd. Returns a 0-dim tensor (fp64 for fp64 inputs, else fp32)."""
    require_device(xv, yv)
    R, Cc = xv.shape
    acc_dt = torch.float64 if xv.dtype == torch.float64 else torch.float32
    slabs = int(lib.gcrnn_batch_time_mse_slabs(R, Cc))
    part = torch.empty((slabs, 2, Cc), dtype=acc_dt, device=xv.device)
    out = torch.empty((1,), dtype=acc_dt, device=xv.device)
    check(lib.gcrnn_batch_time_mse(dtype_code(xv.dtype), _p(xv), _p(yv), _p(part), _p(out), R, Cc, _stream()), 'batch_time_mse')
    return out[0]


CROSS_ENTROPY_MAX_CLASSES = 1024                   # GCRNN_CROSS_ENTROPY_MAX_CLASSES: a row lives in one wave's registers
_CE_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


def cross_entropy_supported(logits):
    """Whether gcrnn_cross_entropy takes these logits: a device matrix [B][C] of f32 / f64 / bf16 with 1 <= C <= 1024, B >= 1."""
    return bool(logits.is_cuda and logits.dim() == 2 and logits.dtype in _CE_DTYPES and logits.shape[0] >= 1
                and 1 <= logits.shape[1] <= CROSS_ENTROPY_MAX_CLASSES)


def _ce_labels(labels, B):
    """int64 labels [B] from int64 or from a floating tensor that holds integers (the reference's dataset keeps labels in the data type
    and casts per batch, train_rnn_quake.py:220), B or B x 1."""
    lab = labels.reshape(-1)
    assert lab.numel() == B, (tuple(labels.shape), B)
    return lab.to(torch.int64).contiguous()


def _ce_launch(zc, lab, want_grad):
    """(loss, hits, grad): 0-dim views of the launch's scratch (accumulation dtype / int64) and the gradient (or None)."""
    B, Cc = zc.shape
    nb = int(lib.gcrnn_cross_entropy_blocks(B, Cc))
    fbuf = torch.empty((nb + 1,), dtype=torch.float64 if zc.dtype == torch.float64 else torch.float32, device=zc.device)
    ibuf = torch.empty((nb + 1,), dtype=torch.int64, device=zc.device)            # [0, nb): per-block sums; [nb]: the result
    grad = torch.empty_like(zc) if want_grad else None
    check(lib.gcrnn_cross_entropy(dtype_code(zc.dtype), _p(zc), _p(lab), _p(grad), _p(fbuf), _p(ibuf),
                                  C.c_void_p(fbuf.data_ptr() + nb * fbuf.element_size()), C.c_void_p(ibuf.data_ptr() + nb * 8),
                                  B, Cc, 1.0 / B, _stream()), 'cross_entropy')
    return fbuf[nb], ibuf[nb], grad


class _CrossEntropy(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean, no weights) with the gradient and the argmax hit count produced by the same launch."""

    @staticmethod
    def forward(ctx, logits, lab):
        zc = logits.contiguous()
        want = ctx.needs_input_grad[0]
        loss, hits, grad = _ce_launch(zc, lab, want)
        ctx.grad = grad
        ctx.used = False
        ctx.operands = (zc, lab) if want else None     # (references: a second backward recomputes the gradient from them)
        ctx.mark_non_differentiable(hits)
        return loss, hits                              # (the accumulation dtype: fp32 for bf16 logits -- a bf16 loss would drop 16 of its bits)

    @staticmethod
    def backward(ctx, gout, _ghits):
        if ctx.operands is None:
            return None, None
        if ctx.used:
            # (as _L1Loss: the buffer was scaled in place and handed out by the first backward; a second backward over a retained graph gets a
            #  FRESH gradient from the saved operands, scaled by its own upstream)
            zc, lab = ctx.operands
            g = _ce_launch(zc, lab, True)[2]
        else:
            g, ctx.grad = ctx.grad, None               # handed out: the only reference left is the caller's (AccumulateGrad may keep it as .grad)
        ctx.used = True
        r = gout.detach().to(torch.float64 if g.dtype == torch.float64 else torch.float32).reshape(1).contiguous()
        if g.data_ptr() % 16 == 0:
            check(lib.gcrnn_scale_unless_one(dtype_code(g.dtype), _p(g), _p(r), g.numel(), _stream()), 'scale_unless_one')
        else:
            g.mul_(r.to(g.dtype))
        return g, None


def cross_entropy(logits, labels, return_hits=False):
    """Mean cross-entropy of logits [B][C] against integer labels [B] (int64, or a floating tensor holding integers) =
    torch.nn.CrossEntropyLoss() with its defaults, on the one-pass HIP kernel; differentiable in the logits; a 0-dim device tensor in
    the logits' dtype (fp32 for bf16 logits: the accumulation type). return_hits=True also
    returns the number of rows whose argmax (first maximal index) equals the label, a 0-dim int64 device tensor of the SAME launch.
    Labels outside [0, C) -- ignore_index = -100 included: not supported -- give a NaN loss and NaN gradient rows. Logits the kernel
    does not take (see cross_entropy_supported; C > 1024, other dtypes) go through torch's own expressions."""
    require_device(logits, labels)
    assert logits.dim() == 2, tuple(logits.shape)
    lab = _ce_labels(labels, logits.shape[0])
    if cross_entropy_supported(logits):
        loss, hits = _CrossEntropy.apply(logits, lab)
    else:
        loss = torch.nn.functional.cross_entropy(logits, lab)
        hits = (torch.argmax(logits.detach(), dim=1) == lab).sum() if return_hits else None
    return (loss, hits) if return_hits else loss


def accuracy(logits, labels):
    """Fraction of rows whose argmax (first maximal index, torch.argmax's rule) equals the label (reference QuakeData.evaluate,
    dataTools.py:1564-1586): the cross-entropy kernel without a gradient. 0-dim device tensor, fp64 for fp64 logits, else fp32."""
    require_device(logits, labels)
    assert logits.dim() == 2, tuple(logits.shape)
    B = logits.shape[0]
    lab = _ce_labels(labels, B)
    out_dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    if cross_entropy_supported(logits):
        hits = _ce_launch(logits.detach().contiguous(), lab, False)[1]
    else:
        hits = (torch.argmax(logits.detach(), dim=1) == lab).sum()
    return hits.to(out_dt) / B


# ------------------------------------------------------------------------------------------ row-linear layers
class _RowLinear(torch.autograd.Function):
    """y = x W^T (+ b) over a huge number of rows (x: R x in; R = T*N*B node-rows of the per-node head and of the
    attention projections). The weight gradient dW = dy^T x reduces over R: a single out x R x in GEMM / GEMV with
    out, in ~ 1..64 and R ~ 1e5..1e7 is a shape the BLAS back ends handle badly (measured: 4.3 ms per call in fp64
    for 1 x 40000 x 20), so the reduction is split into R/C-deep batched GEMMs followed by a sum over the C chunks."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        y = x @ w.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        R = x.shape[0]
        dx = dy @ w if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1]:
            C = max(1, min(256, R // 512))
            Rc = (R // C) * C
            dw = torch.bmm(dy[:Rc].reshape(C, R // C, -1).transpose(1, 2), x[:Rc].reshape(C, R // C, -1)).sum(0)
            if Rc < R:
                dw = dw + dy[Rc:].t() @ x[Rc:]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db


def row_linear(x2d, weight, bias=None):
    return _RowLinear.apply(x2d, weight, bias)


# ------------------------------------------------------------------------------------------ edge gate (attention)
class _EdgeAttention(torch.autograd.Function):
    """y[t, n] = sum_m softmax_row_m(LeakyReLU(s1[n] + s2[m])) (S+I)[m, n] Wx[t, m] on the CSR support (reference
    graphAttention, graphML.py:605-625). Wx: [T][N][B][F], s1 / s2: [T][N][B]."""

    @staticmethod
    def forward(ctx, Wx, s1, s2, graph, e, slope):
        Wx, s1, s2 = Wx.contiguous(), s1.contiguous(), s2.contiguous()
        require_device(Wx, s1, s2)
        T, N, B, F = Wx.shape
        m = graph.mask
        val = graph.mask_vals[e].to(Wx.dtype)
        trp, trow, tpos, _ = graph.mask_transposed()
        alpha = torch.empty((T, m.nnz, B), dtype=Wx.dtype, device=Wx.device)
        y = torch.empty_like(Wx)
        check(lib.gcrnn_attention_forward(dtype_code(Wx.dtype), _p(m.rowptr), _p(m.col), _p(val), _p(trp), _p(trow),
                                          _p(tpos), _p(Wx), _p(s1), _p(s2), _p(alpha), _p(y), T, N, B, F, m.nnz,
                                          float(slope), _stream()), 'attention_forward')
        ctx.save_for_backward(Wx, s1, s2, alpha, val)
        ctx.graph, ctx.slope = graph, float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        Wx, s1, s2, alpha, val = ctx.saved_tensors
        T, N, B, F = Wx.shape
        m = ctx.graph.mask
        trp, trow, tpos, erow = ctx.graph.mask_transposed()
        dy = dy.contiguous()
        dWx = torch.empty_like(Wx)
        ds1 = torch.empty_like(s1)
        ds2 = torch.empty_like(s2)
        dz = torch.empty_like(alpha)
        check(lib.gcrnn_attention_backward(dtype_code(Wx.dtype), _p(m.rowptr), _p(m.col), _p(val), _p(erow), _p(trp),
                                           _p(tpos), _p(Wx), _p(s1), _p(s2), _p(alpha), _p(dy), _p(dWx), _p(ds1), _p(ds2), _p(dz),
                                           T, N, B, F, m.nnz, ctx.slope, _stream()), 'attention_backward')
        return dWx, ds1, ds2, None, None, None


def edge_attention(Wx, s1, s2, graph, e=0, negative_slope=0.2):
    return _EdgeAttention.apply(Wx, s1, s2, graph, e, negative_slope)


# ------------------------------------------------------------------------------------------ hipGraph replay
class FusedForwardGraph(object):
    """The fused forward of one fixed problem (shapes, graph) captured as a hipGraph: pack -> gate pre-passes ->
    T step launches become one graph launch per call (re-captured when a parameter of the cell has changed since). The capture runs on the CALLER's tensors when they are given
    (zero-copy: refill X / h0 in place, or keep feeding the same resident batch, and call the runner with no arguments);
    without them the runner owns static inputs and `runner(X, h0)` copies into them first. The output tensor is reused
    between calls (clone it if it must survive the next replay).

        runner = FusedForwardGraph(cell, B, T, X=X, h0=h0);  H = runner()          # replays on X, h0 as they are now
        runner = FusedForwardGraph(cell, B, T);              H = runner(X2, h02)   # copies, then replays
    """

    def __init__(self, cell, B, T, device=None, X=None, h0=None):
        dev = device if device is not None else cell.weight_A.device
        self.cell = cell
        self.X = X if X is not None else torch.zeros((B, T, cell.G, cell.N), dtype=torch.bfloat16, device=dev)
        self.h0 = h0 if h0 is not None else torch.zeros((B, cell.F, cell.N), dtype=torch.bfloat16, device=dev)
        assert tuple(self.X.shape) == (B, T, cell.G, cell.N) and self.X.is_contiguous() and self.h0.is_contiguous()
        cell.graph.fused_plan()                                   # host-side preparation happens outside the capture
        self._dev = dev
        self._stream = torch.cuda.Stream(device=dev)
        # the fused forward of THIS cell: node- and edge-gated cells have their own (a runner that replayed the un-gated / time-gated path for them
        # would compute another cell)
        with torch.no_grad():
            if cell.spatial_gating == 'node' and cell._use_fused_node(self.X, self.h0):
                self._forward = cell._forward_fused_node
            elif cell.spatial_gating == 'edge' and cell._use_fused_edge(self.X, self.h0):
                self._forward = cell._forward_fused_edge
            elif cell.spatial_gating is None and cell._use_fused(self.X, self.h0):
                self._forward = cell._forward_fused
            elif cell._state_padded(self.X, self.h0) is not None:
                self._forward = lambda X_, h0_: cell(X_, h0_)      # (a state width between the kernels': the zero-padded shadow cell, pads captured with it)
            else:
                raise ValueError('FusedForwardGraph: this cell / problem does not run on the fused forward kernels (bf16, tanh, N <= 1024, F <= 64)')
        self._capture()

    def _capture(self):
        """Warm-up and capture on ONE side stream. The capture records the parameter packs too (ops._cached_pack never answers from its cache
        during a capture), so every replay packs from the LIVE parameters: in-place updates, optimiser steps through raw pointers and `.data`
        writes are all seen without capturing again. Only a parameter whose STORAGE was replaced (`p.data = t`, `.to(...)`) needs a new capture:
        the graph holds the old pointers."""
        cell, dev, s = self.cell, self._dev, self._stream
        with torch.no_grad():
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(2):                                # warm-up on the side stream (allocator, func attributes)
                    self._forward(self.X, self.h0)
            torch.cuda.current_stream(dev).wait_stream(s)
            self._ptrs = tuple((p.data_ptr(), p.dtype, tuple(p.shape)) for p in cell.parameters())
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=s):
                self.H = self._forward(self.X, self.h0)

    def __call__(self, X=None, h0=None):
        if X is not None and X.data_ptr() != self.X.data_ptr():
            self.X.copy_(X)
        if h0 is not None and h0.data_ptr() != self.h0.data_ptr():
            self.h0.copy_(h0)
        if self._ptrs != tuple((p.data_ptr(), p.dtype, tuple(p.shape)) for p in self.cell.parameters()):
            self._capture()                                       # a parameter's storage was replaced: the graph holds the old pointer
        self.graph.replay()
        return self.H
