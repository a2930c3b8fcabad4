"""Graph-ML primitives of the GCRNN hot path on MI355X (HIP kernels behind include/gcrnn.h).

Mirrors the public surface of the reference's Utils/graphML.py for the hot path
only: same names, positional signatures, parameter
names and shapes, `addGSO`, state_dict keys and AssertionError conventions.

    LSIGF(h, S, x, b=None)                                    reference graphML.py:47-140
    GraphFilter(G, F, K, E=1, bias=True)                      reference graphML.py:1086-1205
    GraphAttentional(G, F, K, E=1, nonlinearity, concatenate) reference graphML.py:1999-2128
    NoPool(nInputNodes, nOutputNodes, nHops)                  reference graphML.py:906-944
    GGCRNNCell(G, F, Kin, Kst, sigma, time_gating, spatial_gating, E, bias)
                                                              reference graphML.py:2130-2427

Differences (all documented in DESIGN.md): the GSO is converted to CSR once in
`addGSO` (the dense tensor is kept only as a buffer for checkpoint/inspection);
data runs in a node-major layout internally; `.to(device)` moves the graph too
(the reference does not, architectures.py:1638-1645); inputs must live on a ROCm
device -- there is no CPU path.
"""
import math
import os

import torch
import torch.nn as nn

from .. import ops
from ..graph import GraphOperator, as_operator

zeroTolerance = 1e-9   # reference graphML.py:42
infiniteNumber = 1e12  # reference graphML.py:43


def LSIGF(h, S, x, b=None):
    """y = sum_e sum_k h[:, e, k, :] (x S_e^k) + b   --  drop-in for reference LSIGF (graphML.py:47-140).

    h: F x E x K x G, S: E x N x N dense tensor (or a GraphOperator), x: B x G x N, b: F x 1.
    Returns B x F x N. Shape errors raise AssertionError as in the reference (graphML.py:99-104).
    """
    F, E, K, G = h.shape
    graph = as_operator(S)
    assert graph.E == E
    N = graph.N
    B = x.shape[0]
    assert x.shape[1] == G
    assert x.shape[2] == N
    Xn = ops.pack_node_major(x.reshape(B, 1, G, N))
    if graph.device != x.device:
        graph = graph.to(x.device)
    Yn = ops.lsigf_node_major(Xn, h, b, graph, 1.0)
    return ops.unpack_node_major(Yn).reshape(B, F, N)


class GraphFilter(nn.Module):
    """Linear graph filter layer; parameters `weight` F x E x K x G, `bias` F x 1 (reference graphML.py:1086-1205)."""

    def __init__(self, G, F, K, E=1, bias=True):
        super().__init__()
        self.G, self.F, self.K, self.E = G, F, K, E
        self.S = None
        self.graph = None
        self.weight = nn.parameter.Parameter(torch.empty(F, E, K, G))
        if bias:
            self.bias = nn.parameter.Parameter(torch.empty(F, 1))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.G * self.K)          # reference graphML.py:1159-1164
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)
        ops.parameters_changed()                        # (.data writes do not move the version counters the packed-parameter cache keys on)

    def addGSO(self, S):
        graph = as_operator(S)
        assert graph.E == self.E
        self.N = graph.N
        self.S = S
        self.graph = graph

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.graph is not None:
            self.graph = self.graph.to(self.weight.device)
        return self

    def forward_node_major(self, Xn):
        return ops.lsigf_node_major(Xn, self.weight, self.bias, self.graph, 1.0)

    def forward(self, x):
        B, F, Nin = x.shape
        if Nin < self.N:                                 # zero padding, reference graphML.py:1181-1185
            x = torch.cat((x, torch.zeros(B, F, self.N - Nin, dtype=x.dtype, device=x.device)), dim=2)
        u = LSIGF(self.weight, self.graph, x, self.bias)
        if Nin < self.N:                                 # reference graphML.py:1192-1193
            u = u[:, :, :Nin]
        return u

    def extra_repr(self):
        return 'in_features=%d, out_features=%d, filter_taps=%d, edge_features=%d, bias=%s, %s' % (
            self.G, self.F, self.K, self.E, self.bias is not None,
            'GSO stored' if self.graph is not None else 'no GSO stored')


class NoPool(nn.Module):
    """Pooling layer that does no pooling (reference graphML.py:906-944): same signature as the pooling layers, identity forward."""

    def __init__(self, nInputNodes, nOutputNodes, nHops):
        super().__init__()
        self.nInputNodes = nInputNodes
        self.nOutputNodes = nOutputNodes
        self.nHops = nHops
        self.neighborhood = None

    def addGSO(self, GSO):
        pass

    def forward(self, x):
        assert x.shape[2] == self.nInputNodes
        assert x.shape[2] >= self.nOutputNodes
        return x

    def extra_repr(self):
        return 'in_dim=%d, out_dim=%d, number_hops = %d' % (self.nInputNodes, self.nOutputNodes, self.nHops) + 'no neighborhood needed'


class MaxPoolLocal(nn.Module):
    """Node-selecting pooling (reference graphML.py:946-1084) is not provided: constructing it raises."""

    def __init__(self, nInputNodes, nOutputNodes, nHops):
        raise NotImplementedError('MaxPoolLocal: pooling that selects nodes is not implemented; use NoPool with nSelectedNodes = [N, ...]')


def _graph_attention_node_major(u, mixer, weight, graph, negative_slope=0.2):
    """GAT on the CSR support of S + I (reference graphAttention, graphML.py:521-627), node-major.

    u: [T][N][B][G]; mixer: K x E x 2F; weight: K x E x F x G  ->  [T][N][B][K*F] (heads concatenated, pre-ReLU).
    Edge (m, n) of the support carries e = LeakyReLU(a1.Wx_n + a2.Wx_m); alpha = softmax over the
    neighbours n of row m; y_n = sum_m Wx_m (S+I)[m, n] alpha[m, n].
    """
    K, E, F, _ = weight.shape
    if u.dtype == torch.bfloat16:      # (the stand-alone attention kernels are fp32 / fp64: a bf16 layer is evaluated in fp32 and rounded once)
        return _graph_attention_node_major(u.float(), mixer.float(), weight.float(), graph, negative_slope).to(torch.bfloat16)
    outs = []
    for k in range(K):
        yk = None
        for e in range(E):
            Wx = ops.row_linear(u.reshape(-1, u.shape[3]), weight[k, e])          # (T N B) x F
            s12 = ops.row_linear(Wx, mixer[k, e].view(2, F))                      # a1 . Wx_n | a2 . Wx_m
            y = ops.edge_attention(Wx.view(*u.shape[:3], F), s12[:, 0].reshape(u.shape[:3]),
                                   s12[:, 1].reshape(u.shape[:3]), graph, e, negative_slope)
            yk = y if yk is None else yk + y
        outs.append(yk)
    return outs[0] if K == 1 else torch.cat(outs, dim=3)


class GraphAttentional(nn.Module):
    """Graph attention layer used as the edge gate (reference graphML.py:1999-2128): `mixer` K x E x 2F, `weight` K x E x F x G."""

    def __init__(self, G, F, K, E=1, nonlinearity=nn.functional.relu, concatenate=True):
        super().__init__()
        self.G, self.F, self.K, self.E = G, F, K, E
        self.S = None
        self.graph = None
        self.nonlinearity = nonlinearity
        self.concatenate = concatenate
        self.mixer = nn.parameter.Parameter(torch.empty(K, E, 2 * F))
        self.weight = nn.parameter.Parameter(torch.empty(K, E, F, G))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.G * self.K)          # reference graphML.py:2069-2073
        self.weight.data.uniform_(-stdv, stdv)
        self.mixer.data.uniform_(-stdv, stdv)
        ops.parameters_changed()

    def addGSO(self, S):
        graph = as_operator(S)
        assert graph.E == self.E
        self.N = graph.N
        self.S = S
        self.graph = graph

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.graph is not None:
            self.graph = self.graph.to(self.weight.device)
        return self

    def forward_node_major(self, un):
        """un: [T][N][B][G] -> [T][N][B][K*F] (concatenate) or [T][N][B][F] (mean)."""
        y = _graph_attention_node_major(un, self.mixer, self.weight, self.graph)
        if self.concatenate:
            return self.nonlinearity(y)                                      # reference graphML.py:2101
        T, N, B, _ = y.shape
        return self.nonlinearity(y.view(T, N, B, self.K, self.F).mean(dim=3))     # reference graphML.py:2110-2112

    def forward(self, x):
        ops.require_device(x)
        B, F, Nin = x.shape
        if Nin < self.N:
            x = torch.cat((x, torch.zeros(B, F, self.N - Nin, dtype=x.dtype, device=x.device)), dim=2)
        un = ops.pack_node_major(x.reshape(B, 1, F, self.N))
        y = ops.unpack_node_major(self.forward_node_major(un)).reshape(B, -1, self.N)
        if Nin < self.N:
            y = y[:, :, :Nin]
        return y

    def extra_repr(self):
        return 'in_features=%d, out_features=%d, attention_heads=%d, edge_features=%d, %s' % (
            self.G, self.F, self.K, self.E,
            ('GSO stored: number_nodes=%d' % self.N) if self.graph is not None else 'no GSO stored')


class GGCRNNCell(nn.Module):
    """Gated graph convolutional recurrent cell (reference graphML.py:2130-2427).

        h_t = sigma( gi_t [ni_t .] (A(S) x_t + b) + gf_t [nf_t .] (B(S) h_{t-1} + b) )

    Parameters: weight_A F x E x Kin x G, weight_B F x E x Kst x F, bias F x 1 (one bias, added by
    both filters). Gate sub-networks are created in addGSO under the reference's names
    (GFL_in/MLP_in/GFL_forget/MLP_forget/GFL_out/MLP_out, GRNN_node_*/GFL_node_*,
    input_attention/forget_attention) so state_dicts are interchangeable. As in the reference every
    gate is computed from (x_t, h0) -- the initial state -- so all gates and A(S)x_t are evaluated for
    the whole sequence in one batched pass before the sequential state recurrence.
    forward(X: B x T x G x N, h0: B x F x N) -> H: B x T x F x N.
    """

    def __init__(self, G, F, Kin, Kst, sigma=nn.Tanh, time_gating=True, spatial_gating=None, E=1, bias=True):
        super().__init__()
        self.G, self.F, self.Kin, self.Kst, self.E = G, F, Kin, Kst, E
        self.S = None
        self.graph = None
        self.weight_A = nn.parameter.Parameter(torch.empty(F, E, Kin, G))
        self.weight_B = nn.parameter.Parameter(torch.empty(F, E, Kst, F))
        self.sigma = sigma
        self.time_gating = time_gating
        self.spatial_gating = spatial_gating
        self.bias_flag = bias
        if bias:
            self.bias = nn.parameter.Parameter(torch.empty(F, 1))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.G * self.Kin)        # all three with the INPUT filter's stdv (graphML.py:2229-2235)
        self.weight_A.data.uniform_(-stdv, stdv)
        self.weight_B.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)
        ops.parameters_changed()                        # (.data writes do not move the version counters the packed-parameter cache keys on)

    def _sub_cell(self):
        c = GGCRNNCell(self.G, self.F, self.Kin, self.Kst, self.sigma, time_gating=False, E=self.E, bias=self.bias_flag)
        c.addGSO(self.graph)
        return c

    def addGSO(self, S):
        """Store the GSO (dense E x N x N tensor or GraphOperator) and (re-)create the gate sub-networks,
        in the reference's construction order so that seeded initialisation matches (graphML.py:2237-2334)."""
        if isinstance(S, torch.Tensor):
            assert len(S.shape) == 3
            assert S.shape[0] == self.E
            assert S.shape[2] == S.shape[1]
        graph = as_operator(S)
        assert graph.E == self.E
        self.N = graph.N
        self.S = S
        self.graph = graph
        self.__dict__.pop('_pc', None)                     # (the padded-state shadow of _state_padded belongs to the old graph)
        if self.time_gating == True:  # noqa: E712  (the reference compares with ==)
            dimInputMLP = self.N * self.F
            self.GFL_in = self._sub_cell()
            self.MLP_in = nn.Sequential(nn.Linear(dimInputMLP, 1, bias=self.bias_flag), nn.Sigmoid())
            self.GFL_forget = self._sub_cell()
            self.MLP_forget = nn.Sequential(nn.Linear(dimInputMLP, 1, bias=self.bias_flag), nn.Sigmoid())
            self.GFL_out = self._sub_cell()      # built and saved but never used (graphML.py:2280-2290)
            self.MLP_out = nn.Sequential(nn.Linear(dimInputMLP, 1, bias=self.bias_flag), nn.Sigmoid())
        if self.spatial_gating is not None:
            if self.spatial_gating == 'node':
                self.GRNN_node_in = self._sub_cell()
                gni = GraphFilter(self.F, 1, self.Kst, self.E, self.bias_flag)
                gni.addGSO(self.graph)
                self.GFL_node_in = nn.Sequential(gni, nn.Sigmoid())
                self.GRNN_node_forget = self._sub_cell()
                gnf = GraphFilter(self.F, 1, self.Kst, self.E, self.bias_flag)
                gnf.addGSO(self.graph)
                self.GFL_node_forget = nn.Sequential(gnf, nn.Sigmoid())
            elif self.spatial_gating == 'edge':
                self.input_attention = GraphAttentional(self.F, self.F, 1)
                self.input_attention.addGSO(self.graph)
                self.forget_attention = GraphAttentional(self.F, self.F, 1)
                self.forget_attention.addGSO(self.graph)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.graph is not None:
            self.graph = self.graph.to(self.weight_A.device)
        return self

    def _wants_grad(self, X, h0):
        """Gradient wanted for anything the forward touches: the inputs or ANY parameter of the cell incl. its gate
        sub-networks (a frozen weight_A with trainable weight_B / gates must still record an autograd graph)."""
        return torch.is_grad_enabled() and (X.requires_grad or h0.requires_grad or
                                            any(p.requires_grad for p in self.parameters()))

    # -- node-major building blocks ---------------------------------------------------------------
    def _gate_state(self, Xn, h0n):
        """sigma(A(S)x_t + b + B(S)h0 + b) for all t of an un-gated sub-cell: [T][N][B][F] (graphML.py:2362)."""
        ya = ops.lsigf_node_major(Xn, self.weight_A, self.bias, self.graph, 1.0)
        yb = ops.lsigf_node_major(h0n, self.weight_B, self.bias, self.graph, 1.0)
        return self.sigma(ya + yb)

    @staticmethod
    def _time_gate(sub, mlp, Xn, h0n):
        """sigmoid(Linear(vec_{F,N}(c_t)))  ->  [T][1][B][1]  (graphML.py:2364-2366)."""
        c = sub._gate_state(Xn, h0n)                                   # T x N x B x F
        lin = mlp[0]
        T, N, B, F = c.shape
        wnf = lin.weight.view(F, N).t().contiguous()                    # row-major vec over (f, n) -> [N][F]
        g = torch.einsum('tnbf,nf->tb', c, wnf)
        if lin.bias is not None:
            g = g + lin.bias
        return torch.sigmoid(g).view(T, 1, B, 1)

    @staticmethod
    def _node_gate(sub, gfl, Xn, h0n):
        """sigmoid(GraphFilter_{F->1}(d_t))  ->  [T][N][B][1]  (graphML.py:2383-2389)."""
        d = sub._gate_state(Xn, h0n)
        return torch.sigmoid(gfl[0].forward_node_major(d))

    # -- state widths between the fused kernels' (F = 20 of the reference drivers, kStepPredGRNNs.py:220-222) -------------------
    def _state_padded(self, X, h0):
        """The fused kernels are built for F = 32 / 64 state features. A cell with fewer (un-gated or time-gated, tanh) runs on them
        as the SAME cell with zero-padded state channels: padded rows of the taps / bias / read-out weights are zero, so a padded
        channel computes tanh(0 + 2 * 0) = 0 at every step and feeds nothing back -- results are those of the F-feature cell. Returns
        (shadow cell with F padded, padded h0) or None when the cell does not need / cannot take that route."""
        Fn = nn.functional
        if self.graph is None or self.F in (32, 64) or self.F > 64 or self.spatial_gating not in (None, 'node') or self.E != 1:
            return None
        if self.sigma not in (torch.tanh, Fn.tanh) or X.dtype not in (torch.bfloat16, torch.float32) or h0.dtype != X.dtype:
            return None
        Fp = 32 if self.F <= 32 else 64
        if self.spatial_gating == 'node':
            # node gates (bf16 only: fp32 node-gated cells are the composed path's): the gate cells and their F -> 1 filters pad the same way --
            # a padded gate-cell channel is tanh(0) = 0 under zero filter taps
            if X.dtype != torch.bfloat16 or not ops.fused_node_supported(self.graph, self.N, Fp, self.G, self.Kin, self.Kst, X.dtype, self.E):
                return None
        elif X.dtype == torch.float32:
            if ops.small_supported(self.N, self.graph.fwd[0].nnz, self.G, self.F, self.Kin, self.Kst, X.dtype, self.E) or \
                    self._wants_grad(X, h0) or self.time_gating == True or \
                    not ops.fused_x3_supported(self.graph, self.N, Fp, self.G, self.Kin, self.Kst, X.dtype, self.E):  # noqa: E712
                return None
        elif not ops.fused_supported(self.N, Fp, self.G, self.Kin, self.Kst, X.dtype, self.E):
            return None
        pc = self.__dict__.get('_pc')
        if pc is None or pc.F != Fp or pc.graph is not self.graph or pc.weight_A.dtype != self.weight_A.dtype or \
                pc.weight_A.device != self.weight_A.device:
            with torch.random.fork_rng(devices=[]):          # the shadow's own initialisation must not move the caller's generator
                pc = GGCRNNCell(self.G, Fp, self.Kin, self.Kst, self.sigma, self.time_gating, self.spatial_gating, self.E, self.bias_flag)
                pc.addGSO(self.graph)
            pc = pc.to(device=self.weight_A.device, dtype=self.weight_A.dtype)
            for q in pc.parameters():
                q.requires_grad_(False)
            object.__setattr__(self, '_pc', pc)               # not a sub-module: state_dict keys stay the reference's
        pc.native_layout = bool(getattr(self, 'native_layout', False))
        return pc, Fn.pad(h0, (0, 0, 0, Fp - self.F))

    def _padded_params(self, Fp):
        """This cell's parameters zero-padded to Fp state features (differentiable: autograd drops the padding's gradient)."""
        Fn, F, d, N = nn.functional, self.F, Fp - self.F, self.N
        out = {}
        for name, p in self.named_parameters():
            if name.endswith('weight_A'):
                p = Fn.pad(p, (0, 0, 0, 0, 0, 0, 0, d))
            elif name.endswith('weight_B'):
                p = Fn.pad(p, (0, d, 0, 0, 0, 0, 0, d))
            elif name.endswith('bias') and tuple(p.shape) == (F, 1):
                p = Fn.pad(p, (0, 0, 0, d))
            elif name.endswith('.0.weight') and tuple(p.shape) == (1, F * N):       # gate read-out Linear(N F -> 1), vec over (f, n)
                p = Fn.pad(p.view(1, F, N), (0, 0, 0, d)).reshape(1, Fp * N)
            elif name.endswith('.0.weight') and p.dim() == 4 and p.shape[0] == 1 and p.shape[3] == F:      # node gate's GraphFilter F -> 1: 1 x E x K x F
                p = Fn.pad(p, (0, d))
            out[name] = p
        return out

    def forward(self, X, h0, last_only=False):
        """last_only (an extension the classification model uses in inference): return B x 1 x F x N, the last state only --
        the fused kernels then skip the user-layout store of every other step; the other paths slice."""
        padded = self._state_padded(X, h0)
        if padded is not None:
            from torch.func import functional_call
            pc, h0p = padded
            Hp = functional_call(pc, self._padded_params(pc.F), (X, h0p), {'last_only': last_only})
            H = Hp[:, :, :self.F]
            return H if pc.native_layout else H.contiguous()
        if last_only:
            if (not torch.is_grad_enabled()) and self._use_fused(X, h0):
                return self._forward_fused(X, h0, last_only=True)
            if (not torch.is_grad_enabled()) and self._use_fused_x3(X, h0):
                return ops.fused_cell_forward_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, last_only=True)
            if (not torch.is_grad_enabled()) and self._use_fused_x3(X, h0, time_gated=True):
                return ops.fused_cell_forward_x3_gated(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._fused_gates(), last_only=True)
            if (not torch.is_grad_enabled()) and self._use_fused_node(X, h0):
                return self._forward_fused_node(X, h0, last_only=True)
            if (not torch.is_grad_enabled()) and self._use_fused_x3_node(X, h0):
                return ops.fused_node_cell_forward_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._node_gate_params(),
                                                      self._fused_gates() if self.time_gating == True else None, last_only=True)  # noqa: E712
            if (not torch.is_grad_enabled()) and self._use_fused_edge(X, h0):
                return self._forward_fused_edge(X, h0, last_only=True)
            if self._use_small_edge(X, h0):
                return self._forward_small_edge(X, h0, last_only=True)
            if self._use_small(X, h0) and not os.environ.get('GCRNN_NO_SMALL_HEAD') and self._small_last_state_pays(X):
                # the matrix-core kernel stores the last state alone (ops.small_cell_forward); GCRNN_NO_SMALL_HEAD=1: the slice below (A/B)
                assert h0.shape[0] == X.shape[0] and X.shape[2] == self.G and X.shape[3] == self.N
                ops.require_device(X, h0, self.weight_A)
                return self._forward_small(X, h0, last_only=True)
            return self.forward(X, h0)[:, -1:]
        assert h0.shape[0] == X.shape[0]
        ops.require_device(X, h0, self.weight_A)
        B, T, F_in, N = X.shape
        assert F_in == self.G and N == self.N
        if self._use_fused_training(X, h0):
            Xp, wA = ops.fused_pad_operands(X, self.weight_A)          # G < 32 (the drivers' G = 1): zero-padded channels
            tgates = self._fused_gates() if self.time_gating == True else None  # noqa: E712
            if self.spatial_gating == 'node':
                return ops.fused_node_cell_train(Xp, h0, wA, self.weight_B, self.bias, self.graph, self._node_gate_params(pad=True), tgates)
            if self.spatial_gating == 'edge':
                return ops.fused_edge_cell_train(Xp, h0, wA, self.weight_B, self.bias, self.graph,
                                                 (self.input_attention.mixer, self.input_attention.weight),
                                                 (self.forget_attention.mixer, self.forget_attention.weight), tgates)
            return ops.fused_cell_train(Xp, h0, wA, self.weight_B, self.bias, self.graph, tgates)
        if self._use_fused(X, h0):
            return self._forward_fused(X, h0)
        if self._use_fused_x3_training(X, h0):
            return ops.fused_cell_train_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph)
        if self._use_fused_x3_training(X, h0, time_gated=True):
            return ops.fused_cell_train_x3_gated(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._fused_gates())
        if self._use_fused_node(X, h0):
            return self._forward_fused_node(X, h0)
        if self._use_fused_edge(X, h0):
            return self._forward_fused_edge(X, h0)
        if self._use_fused_x3(X, h0):
            return ops.fused_cell_forward_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph)
        if self._use_fused_x3(X, h0, time_gated=True):
            return ops.fused_cell_forward_x3_gated(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._fused_gates())
        if self._use_fused_x3_node(X, h0):
            return ops.fused_node_cell_forward_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._node_gate_params(),
                                                  self._fused_gates() if self.time_gating == True else None)  # noqa: E712
        if self._use_fused_x3_edge(X, h0):
            return ops.fused_edge_cell_forward_x3(X, h0, self.weight_A, self.weight_B, self.bias, self.graph,
                                                  self.input_attention.forward_node_major, self.forget_attention.forward_node_major,
                                                  self._fused_gates() if self.time_gating == True else None)  # noqa: E712
        if self._use_small_edge(X, h0):
            return self._forward_small_edge(X, h0)
        if self._use_small_edge_training(X, h0):
            return self._forward_small_edge(X, h0, train=True)
        if self._use_small(X, h0):
            return self._forward_small(X, h0)
        if self._use_small_training(X, h0):
            return self._forward_small(X, h0, train=True)
        if self._use_horner(X, h0):
            return self._forward_horner(X, h0)
        if self.weight_A.dtype == torch.bfloat16:
            # bf16 parameters in a variant / shape without bf16 kernels: the composed path has fp32 and fp64 kernels only, so it runs on
            # fp32 views of the parameters (differentiable casts: gradients reach the bf16 parameters) and returns bf16 states
            from torch.func import functional_call
            p32 = {k: v.float() for k, v in self.named_parameters()}
            return functional_call(self, p32, (X.float(), h0.float())).to(torch.bfloat16)
        if X.dtype != self.weight_A.dtype:      # e.g. bf16 batches meeting fp32 master weights in a variant without fused
            X, h0 = X.to(self.weight_A.dtype), h0.to(self.weight_A.dtype)      # kernels: the composed path runs in the parameters' dtype
        Xn = ops.pack_node_major(X)                                     # T x N x B x G
        h0n = ops.pack_node_major(h0.reshape(B, 1, self.F, N))          # 1 x N x B x F
        ya = ops.lsigf_node_major(Xn, self.weight_A, self.bias, self.graph, 1.0)      # all t at once
        gi = gf = None
        if self.time_gating == True:  # noqa: E712
            gi = self._time_gate(self.GFL_in, self.MLP_in, Xn, h0n)
            gf = self._time_gate(self.GFL_forget, self.MLP_forget, Xn, h0n)
        if self.spatial_gating == 'node':
            ni = self._node_gate(self.GRNN_node_in, self.GFL_node_in, Xn, h0n)
            nf = self._node_gate(self.GRNN_node_forget, self.GFL_node_forget, Xn, h0n)
            ya = ni * ya
        elif self.spatial_gating == 'edge':
            ya = self.input_attention.forward_node_major(ya)
        if gi is not None:
            ya = gi * ya
        h = h0n
        Hs = []
        for t in range(T):
            yb = ops.lsigf_node_major(h, self.weight_B, self.bias, self.graph, 1.0)   # 1 x N x B x F
            if self.spatial_gating == 'node':
                yb = nf[t:t + 1] * yb
            elif self.spatial_gating == 'edge':
                yb = self.forget_attention.forward_node_major(yb)
            if gf is not None:
                yb = gf[t:t + 1] * yb
            h = self.sigma(ya[t:t + 1] + yb)
            Hs.append(h)
        Hn = torch.cat(Hs, dim=0)                                       # T x N x B x F
        return ops.unpack_node_major(Hn)

    # -- streaming inference in Horner form (any size, fp32 / fp64, un-gated / time-gated) ------------------
    def _use_horner(self, X, h0):
        if self._wants_grad(X, h0):
            return False            # BPTT runs on the LSIGF autograd nodes
        if X.dtype == torch.bfloat16 and (self.time_gating == True or self.F % 8):  # noqa: E712  (gates are fp32 / fp64 code; 16-byte bf16 rows)
            return False
        return self.spatial_gating is None and self.E == 1 and \
            X.dtype in (torch.float32, torch.float64, torch.bfloat16) and self.weight_A.dtype == X.dtype and h0.dtype == X.dtype

    def _forward_horner(self, X, h0):
        """Taps and shifts act on different axes, so  pre_t = sum_k P^k (gi x_t A_k^T + gf h_{t-1} B_k^T) + (gi + gf) b  is
        evaluated as  acc <- P acc + u_k  (k = K-1 .. 0): K-1 hops over F channels per step, x and h sharing them,
        instead of the reference order's 2 (K-1) hops over G + F channels (graphML.py:118-135 applied twice per step).
        Every hop is one accumulate-SpMM pass over the [N][B F] state (ops.spmm_raw -> gcrnn_spmm_ex); the last hop's
        epilogue adds the bias and applies tanh, writing h_t in place. Taps: one matrix-core pass for all K taps of a step
        in bf16 (gcrnn_taps_bf16_forward), the LDS-tiled tap kernel (gcrnn_taps_forward) in fp32 / fp64 -- no library GEMM."""
        B, T, G, N = X.shape
        F, Kin, Kst = self.F, self.Kin, self.Kst
        K = max(Kin, Kst)
        Xn = ops.pack_node_major(X)                                     # T x N x B x G
        h = ops.pack_node_major(h0.reshape(B, 1, F, N))                 # 1 x N x B x F
        gi = gf = None
        if self.time_gating == True:  # noqa: E712
            gi = self._time_gate(self.GFL_in, self.MLP_in, Xn, h)       # T x 1 x B x 1
            gf = self._time_gate(self.GFL_forget, self.MLP_forget, Xn, h)
        csr = self.graph.fwd[0]
        Hn = torch.empty((T, N, B, F), dtype=X.dtype, device=X.device)
        tanh_fused = self.sigma in (torch.tanh, nn.functional.tanh) and gi is None
        bvec = self.bias.detach().reshape(-1) if self.bias is not None else None
        if X.dtype == torch.bfloat16:
            bvec = bvec.float() if bvec is not None else None           # the kernels take fp32 bias / CSR weights with bf16 rows
            Gp = 32 if G <= 32 else 64
            wA = self.weight_A
            mfma = G <= 64 and ops.taps_bf16_supported(F, Gp, K)
            if mfma and Gp != G:                                        # the matrix-core taps consume whole 32-feature steps
                Xp = Xn.new_zeros((T, N, B, Gp))
                Xp[..., :G] = Xn
                Xn, wA = Xp, nn.functional.pad(wA, (0, Gp - G))
            for t in range(T):
                if mfma:
                    _, rest = ops.taps_bf16(h, Xn[t:t + 1], wA, self.weight_B, out0=Hn[t:t + 1])     # u_0 -> Hn[t], u_1.. -> rest
                else:
                    # shapes outside the matrix-core tap kernel (F not 32 / 64): fp32 taps on the LDS-tiled kernel, rounded to bf16 rows
                    hf, xf = h.float(), Xn[t:t + 1].float()
                    rest = torch.empty((max(K - 1, 1), 1, N, B, F), dtype=X.dtype, device=X.device)
                    for k in range(K):
                        u = ops.taps_rows(hf, self.weight_B[:, 0, k].float()) if k < Kst else None
                        if k < Kin:
                            u = ops.taps_rows(xf, self.weight_A[:, 0, k].float(), out=u, accumulate=u is not None)
                        (Hn[t:t + 1] if k == 0 else rest[k - 1]).copy_(u)
                acc = rest[K - 2] if K > 1 else None
                for k in range(K - 2, -1, -1):
                    dst = rest[k - 1] if k > 0 else Hn[t:t + 1]
                    ops.spmm_raw(csr, acc, out=dst, accumulate=True, bias=bvec, bias_scale=2.0, tanh=(k == 0 and tanh_fused))
                    acc = dst
                if K == 1 or not tanh_fused:
                    pre = Hn[t:t + 1].float() + (2.0 * bvec.view(1, 1, 1, F) if bvec is not None else 0.0)
                    Hn[t:t + 1] = self.sigma(pre).to(X.dtype)
                h = Hn[t:t + 1]
            return ops.unpack_node_major(Hn)
        if gi is None and ops.taps_mfma_supported(X.dtype, F, F, G):
            # every tap of a step in one launch on the fp32 / fp64 matrix cores, then the same hop chain as the bf16 branch
            for t in range(T):
                _, rest = ops.taps_mfma(h, Xn[t:t + 1], self.weight_A, self.weight_B, out0=Hn[t:t + 1])
                acc = rest[K - 2] if K > 1 else None
                for k in range(K - 2, -1, -1):
                    dst = rest[k - 1] if k > 0 else Hn[t:t + 1]
                    ops.spmm_raw(csr, acc, out=dst, accumulate=True, bias=bvec, bias_scale=2.0, tanh=(k == 0 and tanh_fused))
                    acc = dst
                if K == 1 or not tanh_fused:
                    pre = Hn[t:t + 1] + (2.0 * bvec.view(1, 1, 1, F) if bvec is not None else 0.0)
                    Hn[t:t + 1] = self.sigma(pre)
                h = Hn[t:t + 1]
            return ops.unpack_node_major(Hn)
        wA = [self.weight_A[:, 0, k].contiguous() for k in range(Kin)]  # F x G each
        wB = [self.weight_B[:, 0, k].contiguous() for k in range(Kst)]  # F x F each
        for t in range(T):
            acc = None
            for k in range(K - 1, -1, -1):
                dst = Hn[t:t + 1] if k == 0 else torch.empty((1, N, B, F), dtype=X.dtype, device=X.device)
                first = True
                if k < Kst:
                    ops.taps_rows(h, wB[k], out=dst)
                    if gf is not None:
                        dst.mul_(gf[t:t + 1])
                    first = False
                if k < Kin:
                    if gi is None:
                        ops.taps_rows(Xn[t:t + 1], wA[k], out=dst, accumulate=not first)
                    else:
                        u = ops.taps_rows(Xn[t:t + 1], wA[k]).mul_(gi[t:t + 1])
                        dst.copy_(u) if first else dst.add_(u)
                if acc is not None:
                    ops.spmm_raw(csr, acc, out=dst, accumulate=True, bias=bvec, bias_scale=2.0, tanh=(k == 0 and tanh_fused))
                acc = dst
            if K == 1 or not tanh_fused:
                pre = acc
                if bvec is not None:
                    bb = bvec.view(1, 1, 1, F)
                    pre = pre + (2.0 * bb if gi is None else (gi[t:t + 1] + gf[t:t + 1]) * bb)
                Hn[t:t + 1] = self.sigma(pre)
            h = Hn[t:t + 1]
        return ops.unpack_node_major(Hn)

    # -- small-graph persistent path (fp32 / fp64, un-gated / time-gated, sigma = tanh, inference) -------
    def _small_node_gating_ok(self, X, backward):
        """Per-node gates run on the matrix-core family only (dense GSO in LDS)."""
        return self.spatial_gating == 'node' and \
            ops.small_dense_supported(self.N, self.G, self.F, self.Kin, self.Kst, X.dtype, backward=backward, gated=True)

    # -- conditions the _use_* questions below share ----
    def _sigma_is_tanh(self):
        return self.sigma in (torch.tanh, nn.functional.tanh)

    def _all_fp32(self, X, h0):
        return X.dtype == torch.float32 and h0.dtype == X.dtype and self.weight_A.dtype == X.dtype

    def _small_takes(self, X):
        """The one-launch small-graph kernels take this cell's shapes (the fp32-accurate fused paths leave those to them)."""
        return ops.small_supported(self.N, self.graph.fwd[0].nnz, self.G, self.F, self.Kin, self.Kst, X.dtype, self.E)

    def _attention_fusable(self):
        """The edge gates' attention is the one the fused attention kernels evaluate: one head, one edge feature, concatenated, relu."""
        att = self.input_attention
        return att.K == 1 and att.E == 1 and att.concatenate and att.nonlinearity is nn.functional.relu

    def _use_small(self, X, h0):
        if self._wants_grad(X, h0):
            return False
        if not self._sigma_is_tanh():
            return False
        if self.spatial_gating is not None and not self._small_node_gating_ok(X, False):
            return False
        return self.weight_A.dtype == X.dtype and h0.dtype == X.dtype and self._small_takes(X)

    def _use_small_training(self, X, h0):
        """Small graphs, gradients wanted for parameters / h0, and for X where the BPTT kernels' dx variants take the shape
        (ops.small_input_grad_supported: un-gated, time-gated and node-gated cells): forward and BPTT are one launch each."""
        if not torch.is_grad_enabled():
            return False
        if not self._sigma_is_tanh():
            return False
        if self.spatial_gating is not None and not self._small_node_gating_ok(X, True):
            return False
        if self.weight_A.dtype != X.dtype or h0.dtype != X.dtype:
            return False
        shape = (self.N, self.graph.fwd[0].nnz, self.G, self.F, self.Kin, self.Kst, X.dtype, self.E)
        if X.requires_grad:
            return ops.small_input_grad_supported(*shape, gated=self.time_gating == True or self.spatial_gating is not None,  # noqa: E712
                                                  node_gates=self.spatial_gating is not None)
        return ops.small_training_supported(*shape)

    def _small_time_gates(self, X, h0, train=False):
        """(gi, gf), each [T][B], of a time-gated cell on a small graph; (None, None) without time gating."""
        gi = gf = None
        if self.time_gating == True and ops.small_gates_supported(  # noqa: E712
                self.N, self.G, self.F, self.Kin, self.Kst, X.dtype, backward=train):
            # both gates of every step in one launch on the matrix cores (parameters stacked input | forget)
            gin, gfo = self.GFL_in, self.GFL_forget
            lin_i, lin_f = self.MLP_in[0], self.MLP_forget[0]
            gates = ops.small_time_gates(
                X, h0, torch.stack((gin.weight_A[:, 0], gfo.weight_A[:, 0])), torch.stack((gin.weight_B[:, 0], gfo.weight_B[:, 0])),
                torch.stack((gin.bias.view(-1), gfo.bias.view(-1))) if gin.bias is not None else None,
                torch.stack((lin_i.weight.view(-1), lin_f.weight.view(-1))),
                torch.stack((lin_i.bias.view(()), lin_f.bias.view(()))) if lin_i.bias is not None else None, self.graph)
            gi, gf = gates[0], gates[1]
        elif self.time_gating == True:  # noqa: E712   gates read (x_t, h0) only: one batched pass over all t
            B = X.shape[0]
            Xn = ops.pack_node_major(X)
            h0n = ops.pack_node_major(h0.reshape(B, 1, self.F, self.N))
            gi = self._time_gate(self.GFL_in, self.MLP_in, Xn, h0n).reshape(X.shape[1], B)
            gf = self._time_gate(self.GFL_forget, self.MLP_forget, Xn, h0n).reshape(X.shape[1], B)
        return gi, gf

    def _use_small_edge(self, X, h0):
        """Edge-gated cell (optionally time-gated too) on a small graph, fp32 / fp64, inference: the input branch of all steps in one
        launch, the recurrence in a second (ops.small_edge_cell_forward). GCRNN_NO_SMALL_EDGE=1 switches back to the composed path (A/B)."""
        if self._wants_grad(X, h0) or not self._small_edge_takes(X, h0):
            return False
        dt = X.dtype
        return ops.small_edge_supported(self.N, self.graph.fwd[0].nnz, int(self.graph.mask.nnz), self.G, self.F, self.Kin, self.Kst, dt, self.E)

    def _small_edge_takes(self, X, h0):
        """What the one-launch edge-gated kernels ask of the cell and its tensors, whatever the gradient mode (the shape is asked separately)."""
        if self.spatial_gating != 'edge' or not self._sigma_is_tanh() or os.environ.get('GCRNN_NO_SMALL_EDGE'):
            return False
        if self.graph is None or not self._attention_fusable():
            return False
        dt = X.dtype
        return dt in (torch.float32, torch.float64) and h0.dtype == dt and all(p.dtype == dt for p in self.parameters())

    def _use_small_edge_training(self, X, h0):
        """Edge-gated cell on a small graph, gradients wanted for parameters / h0: the forward of _use_small_edge with every state kept,
        BPTT in two launches (ops.small_edge_cell_train). An X that wants a gradient takes this path only with GCRNN_SMALL_EDGE_DX=1 (read
        at every forward; the kernels' dx variant, ops.small_edge_input_grad_supported) and then counts as wanting one even where nothing
        else does; without the variable it stays on the composed path. GCRNN_NO_SMALL_EDGE=1 switches this path off in either case."""
        if not torch.is_grad_enabled():
            return False
        x_grad = X.requires_grad
        if x_grad and not os.environ.get('GCRNN_SMALL_EDGE_DX'):
            return False
        if not (x_grad or h0.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if not self._small_edge_takes(X, h0):
            return False
        supported = ops.small_edge_input_grad_supported if x_grad else ops.small_edge_training_supported
        return supported(self.N, self.graph.fwd[0].nnz, int(self.graph.mask.nnz), self.G, self.F, self.Kin, self.Kst, X.dtype, self.E)

    def _forward_small_edge(self, X, h0, last_only=False, train=False):
        assert h0.shape[0] == X.shape[0] and X.shape[2] == self.G and X.shape[3] == self.N
        ops.require_device(X, h0, self.weight_A)
        gi, gf = self._small_time_gates(X, h0, train)
        att_in = (self.input_attention.mixer, self.input_attention.weight)
        att_f = (self.forget_attention.mixer, self.forget_attention.weight)
        if train:
            return ops.small_edge_cell_train(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, att_in, att_f, gi, gf)
        return ops.small_edge_cell_forward(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, att_in, att_f, gi, gf, last_only=last_only)

    @staticmethod
    def _small_node_gates_pays(X, train, head):
        """Where the one-launch node gates are no slower than the composed batched pass (the acceptance rule of DESIGN 4.11 / 4.12, new
        median <= off median x (1 + off spread), on tools/small_node_gates_bench.py's 72 rows, DESIGN 4.15: adj59 K = 4 and SBM 80 K = 5,
        F = 20, node and time+node, fp32 / fp64, T = 5 / 20 / 200). 68 rows pass: every training step (1.03x .. 2.1x), every model
        inference (head inside the launches, 1.09x .. 3.8x), every fp64 row and every row at T <= 20. The four that fail are the bare cell's
        fp32 inference at T = 200, which stores every state, this path / the switched-off path in ms: adj59 2.359 / 2.182 and (time+node)
        3.156 / 3.031, SBM 80 4.116 / 3.938 and 5.392 / 5.271 -- two latency-bound launches in a row (64 workgroups of gates, then the
        recurrence) against batched passes that fill the chip at that length. Those rows are taken off the dispatch here; nothing between
        T = 20 and T = 200 was measured, so fp32 cell inference keeps the composed pass from T = 21 up. GCRNN_SMALL_NODE_GATES=all takes them
        all the same (peak memory 67 against 251 MB and 90 against 422 MB, 7 device events against 35 / 41). train: a backward may follow;
        head: called for a head inside the launches (_small_linear_head, regress_gnn, classify_gnn)."""
        return train or head or X.dtype != torch.float32 or X.shape[1] <= 20

    def _use_small_node_gates(self, X, train, head):
        """Node gates of a cell on the small matrix-core path in one launch forward, one backward (ops.small_node_gates):
        E = 1, every gate parameter in the input's dtype, shapes by ops.small_node_gates_supported, rows by _small_node_gates_pays
        (GCRNN_SMALL_NODE_GATES=all: every supported row). GCRNN_NO_SMALL_NODE_GATES=1 switches back to the composed batched pass
        (A/B). Both variables are read at every call."""
        if os.environ.get('GCRNN_NO_SMALL_NODE_GATES') or self.E != 1 or not self._sigma_is_tanh():
            return False
        subs = (self.GRNN_node_in, self.GRNN_node_forget, self.GFL_node_in[0], self.GFL_node_forget[0])
        if any(p.dtype != X.dtype for m in subs for p in m.parameters()):
            return False
        if os.environ.get('GCRNN_SMALL_NODE_GATES') != 'all' and not self._small_node_gates_pays(X, train, head):
            return False
        return ops.small_node_gates_supported(self.N, self.G, self.F, self.Kin, self.Kst, X.dtype, backward=train)

    def _small_gates(self, X, h0, train=False, head=False):
        """(gi, gf) as the one-launch recurrence takes them: None, [T][B] time gates, or [B][T][N] node gates (times the time gates)."""
        gi, gf = self._small_time_gates(X, h0, train)
        if self.spatial_gating == 'node' and self._use_small_node_gates(X, train, head):
            # both node gates of every step in one launch (parameters stacked input | forget): gates [2][B][T][N]
            sub_i, sub_f = self.GRNN_node_in, self.GRNN_node_forget
            gfl_i, gfl_f = self.GFL_node_in[0], self.GFL_node_forget[0]
            gates = ops.small_node_gates(
                X, h0, torch.stack((sub_i.weight_A[:, 0], sub_f.weight_A[:, 0])), torch.stack((sub_i.weight_B[:, 0], sub_f.weight_B[:, 0])),
                torch.stack((sub_i.bias.view(-1), sub_f.bias.view(-1))) if sub_i.bias is not None else None,
                torch.stack((gfl_i.weight.reshape(self.Kst, self.F), gfl_f.weight.reshape(self.Kst, self.F))),
                torch.stack((gfl_i.bias.view(()), gfl_f.bias.view(()))) if gfl_i.bias is not None else None, self.graph)
            gi = gates[0] if gi is None else gates[0] * gi.t().unsqueeze(2)
            gf = gates[1] if gf is None else gates[1] * gf.t().unsqueeze(2)
        elif self.spatial_gating == 'node':
            # node gates (graphML.py:2379-2399) from one batched pass over all t; the recurrence takes them per node,
            # multiplied by the time gates when both are on: gates [B][T][N]
            B = X.shape[0]
            Xn = ops.pack_node_major(X)
            h0n = ops.pack_node_major(h0.reshape(B, 1, self.F, self.N))
            ni = self._node_gate(self.GRNN_node_in, self.GFL_node_in, Xn, h0n).squeeze(3).permute(2, 0, 1)      # B x T x N
            nf = self._node_gate(self.GRNN_node_forget, self.GFL_node_forget, Xn, h0n).squeeze(3).permute(2, 0, 1)
            gi = ni if gi is None else ni * gi.t().unsqueeze(2)
            gf = nf if gf is None else nf * gf.t().unsqueeze(2)
        return gi, gf

    def _forward_small(self, X, h0, train=False, last_only=False):
        gi, gf = self._small_gates(X, h0, train)
        if train:
            return ops.small_cell_train(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, gi, gf)
        return ops.small_cell_forward(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, gi, gf, last_only=last_only)

    @staticmethod
    def _small_last_state_pays(X):
        """Inference with the last-state / no-state store of the matrix-core forward: fp64 at every T, fp32 up to T = 20. The kernel's
        extended instantiation keeps more scalars alive across the time loop and spills some of them in fp32: 5.5 us per step against 5.1 us,
        so beyond T = 20 the fp32 inference forward was 2 .. 7 % slower than the all-states launch + slice + Linear and stays there."""
        return X.dtype != torch.float32 or X.shape[1] <= 20

    def classify(self, X, h0, weight, bias):
        """Cell + read-out Linear(F N -> C) on the LAST state (the classification model's head with dimLayersMLP = [C], reference
        architectures.py:1844-1856) inside the small-graph matrix-core launches (ops.small_cell_classify): un-gated, time-gated, node-gated
        and time+node-gated cells, fp32 / fp64. Inference: one launch for recurrence and logits, no state is stored. Training: the forward
        launch stores the states BPTT reads and makes the logits; the BPTT launch starts from dlogits, so the zero-filled dH [B][T][F][N]
        of `H.select(1, -1)` never exists. Returns logits B x C, or None when this cell / input / head does not run on that path (the
        model then continues on forward()). GCRNN_NO_SMALL_HEAD=1 (read at every call) switches it off: A/B against the two-module path."""
        return self._small_linear_head(X, h0, weight, bias, 'GCRNN_NO_SMALL_HEAD', self._readout_weight_ok, self._small_last_state_pays,
                                       ops.small_head_supported, ops.small_cell_classify, ops.SMALL_EDGE_HEAD_LAST,
                                       ops.small_edge_cell_classify)

    def _small_linear_head(self, X, h0, weight, bias, off_switch, weight_ok, pays, supported, fn, edge_kind, edge_fn):
        """classify / regress: the head's output from the matrix-core launches (fn), else -- an edge-gated cell -- from _small_edge_head
        (edge_kind, edge_fn), else None. pays: where the inference launch beats the two-module path, asked once, with `backward` known."""
        backward = self._small_head_backward(X, h0, weight, bias, off_switch, weight_ok)
        if backward is not None and (backward or pays(X)) and self._small_head_takes(X, h0, backward, supported, weight.shape[0]):
            gates = self._small_gates(X, h0, backward, head=True)
            return fn(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, weight, bias, *gates)
        return self._small_edge_head(X, h0, weight, bias, off_switch, weight_ok, edge_kind, edge_fn)

    # -- what the routes of the heads inside the small-graph launches share (classify, regress, regress_gnn, classify_gnn, _small_edge_head)
    def _readout_weight_ok(self, w):
        return w.shape[1] == self.F * self.N

    def _node_weight_ok(self, w):
        return w.shape[1] == self.F and 0 < w.shape[0] <= 8

    def _small_head_backward(self, X, h0, weight, bias, off_switch, weight_ok, edge=False):
        """The first half of a route, no device touched: None to decline, else `backward` -- whether a BPTT launch may follow (the cell
        trains, or the head alone wants a gradient). off_switch: the environment variable that declines, read here at every call;
        weight_ok: the head's test of its 2-D weight; edge: the cell's own questions are the edge-gated kernels' (_use_small_edge /
        _use_small_edge_training), else the matrix-core family's (_use_small / _use_small_training)."""
        if os.environ.get(off_switch) or self.graph is None or self._state_padded(X, h0) is not None:
            return None
        if weight.dim() != 2 or not weight_ok(weight) or weight.dtype != X.dtype or (bias is not None and bias.dtype != X.dtype):
            return None
        head_grad = torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad))
        if self._use_small_edge(X, h0) if edge else self._use_small(X, h0):
            return head_grad
        if self._use_small_edge_training(X, h0) if edge else self._use_small_training(X, h0):
            return True
        return None

    def _small_head_on_device(self, X, h0):
        """The last step of a route that accepts: from here on the device is touched."""
        assert h0.shape[0] == X.shape[0] and X.shape[2] == self.G and X.shape[3] == self.N
        ops.require_device(X, h0, self.weight_A)

    def _small_head_takes(self, X, h0, backward, supported, *head_shape):
        """The second half of a matrix-core route: whether `supported` (the ops query of the head's shapes; head_shape: the head's sizes
        in its order) takes the step, and then that the tensors are where the launches need them. The head's own _pays question is its
        caller's, asked once with `backward`; what follows a yes is the gates, self._small_gates(X, h0, backward, head=True)."""
        gated = self.time_gating == True or self.spatial_gating is not None  # noqa: E712
        if not supported(self.N, self.G, self.F, self.Kin, self.Kst, *head_shape, X.dtype, backward, gated, dx=backward and X.requires_grad):
            return False
        self._small_head_on_device(X, h0)
        return True

    @staticmethod
    def _small_edge_head_pays(X, head_kind):
        """Where the edge-gated recurrence launches with the head inside them are no slower than the two-module path (the acceptance rule of
        DESIGN 4.11 / 4.12 on tools/small_edge_head_bench.py's rows): the read-out in fp32 and fp64 and the per-node head in
        fp32, inference and training step. The per-node head in fp64 fails the rule at T = 20 and T = 200, edge and time+edge, this path /
        the parent tree in ms: inference 0.655 / 0.651 and 6.258 / 6.181, training step 2.244 / 2.226 and 20.13 / 19.94 (SBM 50, F = 20,
        K = 5, B = 100) -- the O N threads that form y_t sit on the step's critical path and cost more than the state stores they replace.
        Those rows are taken off the dispatch here; GCRNN_SMALL_EDGE_HEAD=all takes them all the same (inference memory halves)."""
        return not (head_kind == ops.SMALL_EDGE_HEAD_NODE and X.dtype == torch.float64)

    def _small_edge_head(self, X, h0, weight, bias, off_switch, weight_ok, head_kind, fn):
        """classify / regress of an EDGE-gated cell (optionally time-gated too) on a small graph: the head inside the one-launch edge-gated
        recurrence and its BPTT (ops.small_edge_cell_classify / _regress). Opt-in: GCRNN_SMALL_EDGE_HEAD=1, read at every call
        (the default keeps the two-module path that existing tests pin; a later change may flip it), takes the rows that pay
        (_small_edge_head_pays); GCRNN_SMALL_EDGE_HEAD=all takes every supported row. GCRNN_NO_SMALL_EDGE=1 and the head's own off_switch
        win over it. Returns the head's output, or None to decline: the cell must take _use_small_edge (inference) or
        _use_small_edge_training (training, with its GCRNN_SMALL_EDGE_DX rule for an X that wants a gradient), the head the tests of
        _small_head_backward, the shape ops.small_edge_head_supported."""
        mode = os.environ.get('GCRNN_SMALL_EDGE_HEAD')
        if not mode or self.spatial_gating != 'edge':
            return None
        if mode != 'all' and not self._small_edge_head_pays(X, head_kind):
            return None
        backward = self._small_head_backward(X, h0, weight, bias, off_switch, weight_ok, edge=True)
        if backward is None or not ops.small_edge_head_supported(self.N, self.graph.fwd[0].nnz, int(self.graph.mask.nnz), self.G, self.F,
                                                                 self.Kin, self.Kst, head_kind, weight.shape[0], X.dtype, backward, self.E):
            return None
        self._small_head_on_device(X, h0)
        gi, gf = self._small_time_gates(X, h0, backward)
        att_in = (self.input_attention.mixer, self.input_attention.weight)
        att_f = (self.forget_attention.mixer, self.forget_attention.weight)
        return fn(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, att_in, att_f, weight, bias, gi, gf)

    @staticmethod
    def _small_node_head_pays(X):
        """Inference with the per-node head inside the matrix-core forward (no state stored) against the all-states launch + node_linear:
        every shape. Measured at the k-step driver's shape (N = 80, F = 20, K = 5, B = 100), this path / the parent tree, ms:
        fp32 T = 20 0.190 / 0.197, T = 200 1.793 / 1.807 (device time 1788.0 against 1749.6 + 36.3 us); fp64 T = 20 0.285 / 0.295, T = 200
        2.749 / 2.792. Unlike the last-state store (_small_last_state_pays) the fp32 forward does not lose beyond T = 20, so nothing is taken
        off; a row that fails the acceptance rule would be excluded here."""
        return True

    def regress(self, X, h0, weight, bias):
        """Cell + output head Linear(F -> O) shared by all nodes on EVERY state (the regression model's `multipMlp` head with
        dimLayersMLP = [O], reference architectures.py:1616-1627) inside the small-graph matrix-core launches (ops.small_cell_regress):
        un-gated, time-gated, node-gated and time+node-gated cells, fp32 / fp64. Inference: one launch for recurrence and y, no state is
        stored. Training: the forward launch stores the states BPTT reads and makes y; the BPTT launch forms dH_t = w^T dy_t itself, so the
        dH [B][T][F][N] of the two-module path never exists. Returns y B x T x O x N, or None when this cell / input / head does not run on
        that path (the model then continues on forward()). GCRNN_NO_SMALL_NODE_HEAD=1 (read at every call) switches it off: A/B against the
        two-module path."""
        return self._small_linear_head(X, h0, weight, bias, 'GCRNN_NO_SMALL_NODE_HEAD', self._node_weight_ok, self._small_node_head_pays,
                                       ops.small_node_head_supported, ops.small_cell_regress, ops.SMALL_EDGE_HEAD_NODE,
                                       ops.small_edge_cell_regress)

    @staticmethod
    def _small_gnn_head_pays(X, backward):
        """Where the graph-filter head inside the matrix-core forward is no slower than the two-module path (the acceptance rule of
        DESIGN 4.10 - 4.12 on tools/small_gnn_head_bench.py's rows). backward: the training step (forward launch, adjoint
        kernel, BPTT launch) against the cell's two launches + graph_filter_layer's two; else inference with no state stored against
        the all-states launch + graph_filter_layer. Measured at the k-step driver's shape (N = 80, F = 20, K = K_o = 5, B = 100), this path /
        the switched-off path in one process, median ms. Inference passes in all twelve rows at T >= 20, by 2.8 .. 10.6 % (fp32 un-gated
        T = 200 1.980 / 2.190, fp64 2.889 / 3.163), and stays on at every T. The training step passes in all six rows at T = 200, by
        0.4 .. 2.9 % (fp32 un-gated 6.415 / 6.604, fp64 9.416 / 9.470), and fails in five of six at T = 20, un-gated / time / node:
        fp32 0.769 / 0.758, 1.349 / 1.343, 2.150 / 2.138, fp64 1.060 / 1.031, 1.860 / 1.840 (3.011 / 3.002 passes inside the off spread):
        the adjoint kernel and node_linear's slot kernel are two launches where graph_filter_layer's backward is one, and the dH they
        save is small there. So training is dispatched from T = 200 up, the length it was measured to pay at; shorter sequences keep
        the two-module path (T = 5 is host time and bimodal: nothing is claimed). GCRNN_SMALL_GNN_HEAD=all takes them all the same
        (the training step's peak memory falls by a third: 354.6 against 540.1 MB in fp64 at T = 200)."""
        return not backward or X.shape[1] >= 200

    def regress_gnn(self, X, h0, weight, bias, act):
        """Cell + one graph-filter layer GraphFilter(F -> 1, K_o) + activation on EVERY state (the regression model's Selection-GNN head
        with dimNodeSignals = [F, 1], nFilterTaps = [K_o], NoPool, no MLP; reference architectures.py:1588-1604, 1630-1632) inside the
        small-graph matrix-core launches (ops.small_cell_regress_gnn): un-gated, time-gated, node-gated and time+node-gated cells,
        fp32 / fp64, E = 1. weight: the GraphFilter's F_out x E x K_o x F parameter with F_out = E = 1, bias 1 x 1 or None, act a key of
        ops._GFL_ACTS. Inference: one launch for recurrence and y, no state is stored. Training: the forward launch stores the states
        BPTT reads and makes y; the head's adjoint kernel makes dU [B][T][K_o][N] and the BPTT launch forms dH_t from it, so the
        dH [B][T][F][N] of the two-module path never exists. Returns y B x T x 1 x N, or None when this cell / input / head does not run
        on that path (the model then continues on forward() + SelectionGNN). GCRNN_NO_SMALL_GNN_HEAD=1 (read at every call) switches it
        off: A/B against the two-module path. GCRNN_SMALL_GNN_HEAD=all takes every supported row, also those _small_gnn_head_pays
        leaves to the two-module path (the measurement's own switch)."""
        every = os.environ.get('GCRNN_SMALL_GNN_HEAD') == 'all'
        taps, bias1 = self._gnn_head_params(weight, bias, act)
        backward = None if taps is None else self._small_head_backward(X, h0, taps, bias1, 'GCRNN_NO_SMALL_GNN_HEAD', self._node_weight_ok)
        if backward is None or not self._small_head_takes(X, h0, backward, ops.small_gnn_head_supported, taps.shape[0]):
            return None
        if not (every or self._small_gnn_head_pays(X, backward)):
            return None
        gates = self._small_gates(X, h0, backward, head=True)
        return ops.small_cell_regress_gnn(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, taps, bias1, act, *gates)

    def _gnn_head_params(self, weight, bias, act):
        """(taps [K_o][F], bias [1] or None) of a one-feature graph-filter head as the ops entries take them, from the GraphFilter's
        F_out x E x K_o x F weight and 1 x 1 bias; (None, None) where it is not such a head (F_out = E = 1, act a key of ops._GFL_ACTS)."""
        if weight.dim() != 4 or weight.shape[0] != 1 or weight.shape[1] != 1 or self.E != 1 or act not in ops._GFL_ACTS:
            return None, None
        if bias is not None and bias.numel() != 1:
            return None, None
        # (a view, not weight[0, 0]: the backward of an index is a zero-fill and a copy per level, four launches a step)
        return weight.reshape(weight.shape[2], weight.shape[3]), bias.view(1) if bias is not None else None

    @staticmethod
    def _small_cls_gnn_head_pays(X, backward):
        """Where the graph-filter head and read-out on the last state inside the matrix-core launches are no slower than the two-module
        path (the acceptance rule of DESIGN 4.14, new median <= off median x (1 + off spread), on tools/small_cls_gnn_head_bench.py's rows,
        DESIGN 4.16). backward: the training step (forward launch, BPTT launch seeded from dlogits) against the cell's two launches, the
        zero-filled dH of `select` and graph_filter_layer's two; else inference with no state stored against the last-state launch +
        graph_filter_layer + Linear. Measured at the epicenter driver's shape (adj59, F = 20, K = K_o = 4, C = 11, B = 100), this
        path / the switched-off path in one process, median ms: all 36 rows pass. Inference at T = 20 / 200, un-gated: fp32 0.120 / 0.141
        and 1.050 / 1.059, fp64 0.156 / 0.169 and 1.394 / 1.409; over the twelve rows at T >= 20 it gains 0.8 .. 17 %. The training step at
        T = 20 / 200, un-gated: fp32 0.494 / 0.653 and 3.376 / 3.399, fp64 0.585 / 0.607 and 4.400 / 4.631; over the twelve rows at T >= 20
        it gains 0.6 .. 32 %, the narrowest being fp64 time-gated T = 20, 1.1256 / 1.1323 inside an off spread of 0.5 %. T = 5 rows are
        host time and bimodal (off spreads up to 51 %): reported, nothing claimed. So nothing is taken off the dispatch; a row that fails the
        rule would be excluded here and named with its figures (GCRNN_SMALL_CLS_GNN_HEAD=all would still take it)."""
        return True

    def classify_gnn(self, X, h0, weight, bias, act, lin_weight, lin_bias):
        """Cell + one graph-filter layer GraphFilter(F -> 1, K_o) + activation + Linear(N -> C) on the LAST state (the classification
        model's Selection-GNN head with dimNodeSignals = [F, 1], nFilterTaps = [K_o], NoPool, dimLayersMLP = [C]; reference
        architectures.py:1823-1849) inside the small-graph matrix-core launches (ops.small_cell_classify_gnn): un-gated, time-gated,
        node-gated and time+node-gated cells, fp32 / fp64, E = 1. weight: the GraphFilter's F_out x E x K_o x F parameter with
        F_out = E = 1, bias 1 x 1 or None, act a key of ops._GFL_ACTS, lin_weight C x N, lin_bias C or None. Inference: one launch for
        recurrence and logits, no state is stored. Training: the forward launch stores the states BPTT reads, the head's output and the
        logits; the BPTT launch starts from dlogits, so neither the zero-filled dH [B][T][F][N] of `H.select(1, -1)` nor an adjoint launch
        exists. Returns logits B x C, or None when this cell / input / head does not run on that path (the model then continues on
        forward() + SelectionGNN). GCRNN_NO_SMALL_CLS_GNN_HEAD=1 (read at every call) switches it off: A/B against the two-module path.
        GCRNN_SMALL_CLS_GNN_HEAD=all takes every supported row, also those _small_cls_gnn_head_pays leaves to the two-module path."""
        every = os.environ.get('GCRNN_SMALL_CLS_GNN_HEAD') == 'all'
        taps, bias1 = self._gnn_head_params(weight, bias, act)
        if taps is None or self.graph is None or lin_weight.dim() != 2 or lin_weight.shape[1] != self.N or lin_weight.dtype != X.dtype or \
                (lin_bias is not None and lin_bias.dtype != X.dtype):
            return None
        backward = self._small_head_backward(X, h0, taps, bias1, 'GCRNN_NO_SMALL_CLS_GNN_HEAD', self._node_weight_ok)
        if backward is None or not self._small_head_takes(X, h0, backward, ops.small_cls_gnn_head_supported, taps.shape[0],
                                                          lin_weight.shape[0]):
            return None
        lin_grad = torch.is_grad_enabled() and (lin_weight.requires_grad or (lin_bias is not None and lin_bias.requires_grad))
        if not (every or self._small_cls_gnn_head_pays(X, backward)) or (lin_grad and not backward):
            return None             # (only the read-out wants a gradient: the shape has been asked for an inference launch)
        gates = self._small_gates(X, h0, backward, head=True)
        return ops.small_cell_classify_gnn(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, taps, bias1, lin_weight, lin_bias, act,
                                           *gates)

    # -- fused flagship path (bf16, un-gated / time-gated, sigma = tanh; inference here, training via ops.fused_cell_train) ----
    def _use_fused(self, X, h0):
        if self._wants_grad(X, h0):
            return False            # BPTT runs on the fused training path or the composed path
        if self.spatial_gating is not None or not self._sigma_is_tanh():
            return False
        return ops.fused_supported(self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E) and \
            self.weight_A.dtype in (X.dtype, torch.float32) and h0.dtype == X.dtype

    def _use_fused_node(self, X, h0):
        """Node-gated cell (optionally time-gated too), bf16, inference: fused kernels (gates, A(S)x_t + b and both gate filters for
        all steps at once; the recurrence on the state-only operand with per-node gates in its epilogue)."""
        if self._wants_grad(X, h0) or self.spatial_gating != 'node' or not self._sigma_is_tanh():
            return False
        if self.bias is None and self.time_gating == True:  # noqa: E712
            return False
        return ops.fused_node_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E) and \
            self.weight_A.dtype in (X.dtype, torch.float32) and h0.dtype == X.dtype

    def _node_gate_params(self, pad=False):
        """pad: the gate cells' input taps zero-padded to the kernels' channel count by a differentiable pad (training)."""
        Gp = ops.fused_padded_inputs(self.F, self.G)
        padf = (lambda w: w) if (not pad or Gp == self.G) else (lambda w: nn.functional.pad(w, (0, Gp - self.G)))
        out = {}
        for name, sub, gfl in (('in', self.GRNN_node_in, self.GFL_node_in[0]), ('forget', self.GRNN_node_forget, self.GFL_node_forget[0])):
            out[name] = (padf(sub.weight_A), sub.weight_B, sub.bias, gfl.weight, gfl.bias)
        return out

    def _forward_fused_node(self, X, h0, last_only=False):
        tg = self._fused_gates() if self.time_gating == True else None  # noqa: E712
        return ops.fused_node_cell_forward(X, h0, self.weight_A, self.weight_B, self.bias, self.graph, self._node_gate_params(),
                                           time_gates=tg, last_only=last_only)

    def _use_fused_edge(self, X, h0):
        """Edge-gated cell (optionally time-gated too), bf16, inference: the attention's mixing matrix is folded into the filter taps,
        the x branch runs for all steps at once, every step is a filter pass plus the attention kernel."""
        if self._wants_grad(X, h0) or self.spatial_gating != 'edge' or not self._sigma_is_tanh():
            return False
        if self.bias is None and self.time_gating == True:  # noqa: E712
            return False
        if not self._attention_fusable():
            return False
        return ops.fused_edge_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E) and \
            self.weight_A.dtype in (X.dtype, torch.float32) and h0.dtype == X.dtype

    def _forward_fused_edge(self, X, h0, last_only=False):
        tg = self._fused_gates() if self.time_gating == True else None  # noqa: E712
        return ops.fused_edge_cell_forward(X, h0, self.weight_A, self.weight_B, self.bias, self.graph,
                                           (self.input_attention.mixer, self.input_attention.weight),
                                           (self.forget_attention.mixer, self.forget_attention.weight), time_gates=tg, last_only=last_only)

    def _use_fused_x3(self, X, h0, time_gated=False):
        """fp32 inference of the un-gated cell on the fp32-accurate fused kernels (three bf16 planes per operand): graphs that fit
        the fused kernels, too large for the one-launch small-graph kernels, with one weight on every edge. time_gated=True: the same
        question for the time-gated cell (ops.fused_cell_forward_x3_gated: gates and scaled steps composed from the same kernel)."""
        if self._wants_grad(X, h0):
            return False
        if (self.time_gating == True) != bool(time_gated) or self.spatial_gating is not None or not self._sigma_is_tanh():  # noqa: E712
            return False
        if time_gated and (X.shape[0] > 2048 or os.environ.get('GCRNN_NO_X3_GATED')):
            return False
        if not self._all_fp32(X, h0):
            return False
        if self._small_takes(X):
            return False
        return ops.fused_x3_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E, X.shape[0], X.shape[1])

    def _use_fused_x3_node(self, X, h0):
        """fp32 inference of the NODE-gated cell (with or without time gates) on the fp32-accurate fused kernels (round 5,
        ops.fused_node_cell_forward_x3): the x3 conditions with G == F."""
        if self._wants_grad(X, h0) or self.spatial_gating != 'node' or not self._sigma_is_tanh():
            return False
        if not self._all_fp32(X, h0) or X.shape[0] > 2048:
            return False
        if self._small_takes(X):
            return False
        return ops.fused_node_x3_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E, X.shape[0], X.shape[1])

    def _use_fused_x3_edge(self, X, h0):
        """fp32 inference of the EDGE-gated cell (with or without time gates) with both filters on the fp32-accurate fused kernels (round 5,
        ops.fused_edge_cell_forward_x3; the attentions run on the fp32 CSR edge-softmax kernels): the x3 conditions with G == F."""
        if self._wants_grad(X, h0) or self.spatial_gating != 'edge' or not self._sigma_is_tanh():
            return False
        if not self._all_fp32(X, h0) or X.shape[0] > 2048 or os.environ.get('GCRNN_NO_X3_EDGE'):
            return False
        if self._small_takes(X):
            return False
        return self.G == self.F and ops.fused_x3_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E, X.shape[0], X.shape[1])

    def _use_fused_x3_training(self, X, h0, time_gated=False):
        """fp32 training of the un-gated cell at the north_star's tolerance on the fused kernels (x3 forward, x3 data chain, exact-fp32
        weight gradient): fp32 tensors and parameters, uniform-weight graph (forward and adjoint), gradients for the parameters and h0.
        time_gated=True (r4): the same question for the time-gated cell (ops.fused_cell_train_x3_gated: gradients for every parameter,
        the gates' sub-cells and read-outs included; none for h0)."""
        if not torch.is_grad_enabled() or X.requires_grad:
            return False
        if not (h0.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if (self.time_gating == True) != bool(time_gated) or self.spatial_gating is not None or not self._sigma_is_tanh():  # noqa: E712
            return False
        if not self._all_fp32(X, h0) or os.environ.get('GCRNN_NO_X3_TRAINING'):
            return False
        if self._small_takes(X):
            return False
        if time_gated:
            if h0.requires_grad or self.GFL_in.weight_A.dtype != X.dtype or os.environ.get('GCRNN_NO_X3_GATED'):
                return False
            return ops.fused_x3_time_training_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E, X.shape[0], X.shape[1])
        return ops.fused_x3_training_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E, X.shape[0], X.shape[1])

    def _use_fused_training(self, X, h0):
        """bf16 activations (parameters bf16 or fp32 master weights), plain or time-gated cell, gradients wanted for the
        parameters (and, for the plain cell, optionally h0; X too when G == F): forward and BPTT on the fused kernels."""
        if not torch.is_grad_enabled():
            return False
        if X.requires_grad and (self.spatial_gating is not None or not ops.fused_input_grad_ok(self.F, self.G)):
            return False                                   # dX: un-gated and (r4) time-gated cells with G == F (the input filters' adjoint passes, the gate cells' included)
        if not (h0.requires_grad or X.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if self.spatial_gating == 'node':
            if h0.requires_grad or self.bias is None or self.GRNN_node_in.weight_A.dtype != self.weight_A.dtype or \
                    not ops.fused_node_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, X.dtype, self.E):
                return False
        elif self.spatial_gating == 'edge':
            if h0.requires_grad or not self._attention_fusable() or self.input_attention.weight.dtype != self.weight_A.dtype or \
                    not ops.fused_edge_training_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, self.E):
                return False
        elif self.spatial_gating is not None:
            return False
        if self.time_gating == True:  # noqa: E712   the gates' sub-cells share the cell's shapes; (r4) they hand h0 its gradient when G == F
            if (h0.requires_grad and not ops.fused_input_grad_ok(self.F, self.G)) or self.bias is None or self.GFL_in.weight_A.dtype != self.weight_A.dtype:
                return False
        if not self._sigma_is_tanh() or X.dtype != torch.bfloat16 or h0.dtype != X.dtype:
            return False
        if self.weight_A.dtype not in (torch.bfloat16, torch.float32):
            return False
        return ops.fused_training_supported(self.graph, self.N, self.F, self.G, self.Kin, self.Kst, self.E)

    def _fused_gates(self):
        Gp = ops.fused_padded_inputs(self.F, self.G)
        pad = (lambda w: w) if Gp == self.G else (lambda w: nn.functional.pad(w, (0, Gp - self.G)))
        return {'in': (pad(self.GFL_in.weight_A), self.GFL_in.weight_B, self.GFL_in.bias,
                       self.MLP_in[0].weight, self.MLP_in[0].bias),
                'forget': (pad(self.GFL_forget.weight_A), self.GFL_forget.weight_B, self.GFL_forget.bias,
                           self.MLP_forget[0].weight, self.MLP_forget[0].bias)}

    def _forward_fused(self, X, h0, last_only=False, head=None):
        gates = self._fused_gates() if self.time_gating == True else None  # noqa: E712
        # (G < 32, the drivers' G = 1: the taps are padded here, X by the pack kernel itself -- no padded copy of X)
        return ops.fused_cell_forward(X, h0, ops.fused_pad_taps(self.weight_A), self.weight_B, self.bias, self.graph, gates, last_only=last_only, head=head,
                                      native_out=bool(getattr(self, 'native_layout', False)) and head is None)

    def forward_native(self, xs, h0s=None):
        """The un-gated recurrence on the fused kernels' own layout end to end (inference): xs [T][B][NPad][G] bf16 sequence-major
        (ops.to_sequence_major, or a generator that emits it), h0s [B][NPad][F] or None (zeros) -> hs [T][B][NPad][F] bf16;
        `hs.permute(1, 0, 3, 2)[..., :N]` is H in the reference's B x T x F x N shape (graphML.py:2425-2427) without a copy.
        The module flag `native_layout = True` gives the same view from the ordinary forward(X, h0) (user-layout X in)."""
        assert self.graph is not None and self.time_gating != True and self.spatial_gating is None  # noqa: E712
        assert not torch.is_grad_enabled() or not any(p.requires_grad for p in self.parameters()), 'forward_native is an inference path'
        assert xs.dtype == torch.bfloat16 and self.weight_A.dtype == torch.bfloat16 and self.sigma in (torch.tanh, nn.functional.tanh)
        wA = self.weight_A
        if wA.shape[3] != xs.shape[3]:                   # G < 32: the padded taps of ops.fused_pad_operands
            wA = torch.nn.functional.pad(wA.detach(), (0, xs.shape[3] - wA.shape[3]))
        assert ops.fused_supported(self.N, self.F, xs.shape[3], self.Kin, self.Kst, torch.bfloat16, self.E), 'shape outside the fused kernels'
        return ops.fused_cell_forward_native(xs, h0s, wA, self.weight_B, self.bias, self.graph, self.N)

    def forward_with_head(self, X, h0, weight, bias):
        """Inference of cell + output head Linear(F -> 1) shared by all nodes (the regression model's `multipMlp` head with one
        output, reference architectures.py:1616-1627) with the head fused into a recurrence kernel's epilogue: the wide sequence-resident
        kernel `fused_seq32_kernel` (head variant, ONE launch per forward: ops.fused_wide_head_supported) where it takes the problem, else the
        per-step `fused_step_kernel` (EPI == 6, the head on its h_t store). Returns y: B x T x 1 x N (fp32) without ever writing H in the user
        layout; None when this cell / input does not run on that path."""
        if torch.is_grad_enabled() or not self._use_fused(X, h0) or self.N % 8 != 0 or os.environ.get('GCRNN_NO_FUSED_HEAD'):      # env: A/B switch
            return None
        return self._forward_fused(X, h0, head=(weight, bias))

    def train_with_head(self, X, h0, weight, bias):
        """Training counterpart of forward_with_head: cell + output head Linear(F -> 1) shared by all nodes as ONE autograd node
        (ops.fused_cell_head_train). Forward: the cell's training forward and the head's kernel on H, as the two modules run them. Backward:
        the head's gradient reaches the wide BPTT chain as its factors (w_head, dy) -- dH [B][T][F][N] and its sequence-major copy are never
        allocated, written or read (gcrnn_fused_backward_data_wide_head_bf16) -- and every gradient equals the two-module path's bit for bit.
        Returns y: B x T x 1 x N (bf16), or None when this cell / input does not run on that path: it needs the fused training path
        (_use_fused_training) of the un-gated or time-gated cell, the head's bf16 kernels, a uniform-weight graph and a batch the persistent
        wide chain takes (ops.fused_cell_head_train_supported). GCRNN_NO_HEAD_CHAIN=1 (read at every call) switches it off: A/B against the
        two-module path."""
        if os.environ.get('GCRNN_NO_HEAD_CHAIN') or self.spatial_gating is not None or self.F % 32 != 0 or not self._use_fused_training(X, h0):
            return None
        if tuple(weight.shape) != (1, self.F) or (bias is not None and bias.dtype != weight.dtype):
            return None
        B, T, F_in, N = X.shape
        assert F_in == self.G and N == self.N and h0.shape[0] == B
        if not ops.fused_cell_head_train_supported(self.graph, B, T, N, self.F, max(self.Kin, self.Kst), weight.dtype):
            return None
        Xp, wA = ops.fused_pad_operands(X, self.weight_A)          # G < 32 (the drivers' G = 1): zero-padded channels
        tgates = self._fused_gates() if self.time_gating == True else None  # noqa: E712
        y = ops.fused_cell_head_train(Xp, h0, wA, self.weight_B, self.bias, self.graph, weight, bias, tgates)
        return y.view(B, T, 1, N)

    def extra_repr(self):
        return 'in_features=%d, state_features=%d, taps=(%d,%d), time_gating=%s, spatial_gating=%s, %s' % (
            self.G, self.F, self.Kin, self.Kst, self.time_gating, self.spatial_gating,
            ('GSO stored: number_nodes=%d' % self.N) if self.graph is not None else 'no GSO stored')
