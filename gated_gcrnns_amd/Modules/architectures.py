"""GatedGCRNN architectures on the MI355X-native cell (mirror of the reference's
Modules/architectures.py:1405-1859 for the hot path).

Same positional constructor signatures, attribute names and state_dict keys
(`stateGCRNN.*`, `outputNN.<i>.*`). Output heads: the MLPs (the drivers' 'multipMlp' /
'oneMlp') and the Selection GNN (reference architectures.py:10-177, also stand-alone as
`SelectionGNN`) without node-selecting pooling; every graph-filter layer of it runs as one
HIP launch per pass (ops.graph_filter_layer). Aggregation-GNN heads are not provided. The drivers' plain-RNN
baselines (reference :1861-2149) are `RNNforRegression` / `RNNforClassification` on ops.rnn_sequence.
"""
import numpy as np
import torch
import torch.nn as nn

from ..Utils import graphML as gml
from .. import ops


def _as_gso_tensor(GSO):
    assert len(GSO.shape) == 2 or len(GSO.shape) == 3
    if len(GSO.shape) == 2:
        assert GSO.shape[0] == GSO.shape[1]
        GSO = GSO.reshape([1, GSO.shape[0], GSO.shape[1]])       # 1 x N x N (reference :1501-1506)
    else:
        assert GSO.shape[1] == GSO.shape[2]
    return torch.tensor(np.asarray(GSO)) if not isinstance(GSO, torch.Tensor) else GSO


def _apply_mlp_rows(mlp, x2d):
    """nn.Sequential of Linear / activation modules applied to rows, Linear layers through _RowLinearFn."""
    for layer in mlp:
        if isinstance(layer, nn.Linear):
            x2d = ops.row_linear(x2d, layer.weight, layer.bias)
        else:
            x2d = layer(x2d)
    return x2d


def _to_param_dtype(h, mlp):
    """bf16 states from the fused cell meeting fp32 master weights in a library-GEMM head: compute in the parameters' dtype."""
    for p in mlp.parameters():
        return h if h.dtype == p.dtype else h.to(p.dtype)
    return h


def _build_mlp(dimInputMLP, dimLayersMLP, sigma2, sigma3, bias):
    fc = []
    if len(dimLayersMLP) > 0:
        fc.append(nn.Linear(dimInputMLP, dimLayersMLP[0], bias=bias))
        for l in range(len(dimLayersMLP) - 1):
            fc.append(sigma2())
            fc.append(nn.Linear(dimLayersMLP[l], dimLayersMLP[l + 1], bias=bias))
    if sigma3 is not None:
        fc.append(sigma3())
    return nn.Sequential(*fc)


_FUSED_ACTIVATIONS = {nn.ReLU: 'relu', nn.Tanh: 'tanh', nn.Sigmoid: 'sigmoid'}


class SelectionGNN(nn.Module):
    """Selection GNN (reference architectures.py:10-177): L graph-filter layers (GraphFilter, sigma, pooling) and an MLP on the
    flattened output. Same signature, asserts, state_dict keys (`GFL.<3l>.*`, `MLP.<i>.*`) and seeded initialisation.

    forward(x: B x F[0] x N) -> B x dimLayersMLP[-1] (B x F[-1]*N without an MLP). Each layer is ops.graph_filter_layer on the
    GraphFilter's live parameters with sigma fused when it is ReLU / Tanh / Sigmoid (other modules are applied after it).
    Only NoPool with nSelectedNodes[l] = N is provided: pooling that drops nodes raises NotImplementedError.
    """

    def __init__(self, dimNodeSignals, nFilterTaps, bias, nonlinearity, nSelectedNodes, poolingFunction, poolingSize,
                 dimLayersMLP, GSO):
        super().__init__()
        assert len(dimNodeSignals) == len(nFilterTaps) + 1
        assert len(nSelectedNodes) == len(nFilterTaps)
        assert len(poolingSize) == len(nFilterTaps)
        S = _as_gso_tensor(GSO)
        self.L = len(nFilterTaps)
        self.F = dimNodeSignals
        self.K = nFilterTaps
        self.E = int(S.shape[0])
        self.N = [int(S.shape[1])] + nSelectedNodes
        if poolingFunction is not gml.NoPool or any(n != self.N[0] for n in nSelectedNodes):
            raise NotImplementedError('SelectionGNN: pooling that selects nodes (MaxPoolLocal, nSelectedNodes != N) is not implemented; '
                                      'use poolingFunction=NoPool with nSelectedNodes=[N] * L')
        self.bias = bias
        self.register_buffer('S', S, persistent=False)            # moved by .to(); not in state_dict (as the reference)
        self.sigma = nonlinearity
        self.rho = poolingFunction
        self.alpha = poolingSize
        self.dimLayersMLP = dimLayersMLP
        gfl = []
        for l in range(self.L):                                   # reference :114-129, same construction order
            gfl.append(gml.GraphFilter(self.F[l], self.F[l + 1], self.K[l], self.E, self.bias))
            gfl[3 * l].addGSO(self.S)
            gfl.append(self.sigma())
            gfl.append(self.rho(self.N[l], self.N[l + 1], self.alpha[l]))
            gfl[3 * l + 2].addGSO(self.S)
        self.GFL = nn.Sequential(*gfl)
        fc = []
        if len(self.dimLayersMLP) > 0:                            # reference :133-153
            fc.append(nn.Linear(self.N[-1] * self.F[-1], dimLayersMLP[0], bias=self.bias))
            for l in range(len(dimLayersMLP) - 1):
                fc.append(self.sigma())
                fc.append(nn.Linear(dimLayersMLP[l], dimLayersMLP[l + 1], bias=self.bias))
        self.MLP = nn.Sequential(*fc)

    def forward(self, x):
        assert len(x.shape) == 3
        batchSize = x.shape[0]
        assert x.shape[1] == self.F[0]
        assert x.shape[2] == self.N[0]
        y = x
        for l in range(self.L):
            gf, sigma, pool = self.GFL[3 * l], self.GFL[3 * l + 1], self.GFL[3 * l + 2]
            act = _FUSED_ACTIVATIONS.get(type(sigma))
            y = ops.graph_filter_layer(y, gf.weight, gf.bias, gf.graph, act)
            if act is None:
                y = sigma(y)
            y = pool(y)
        y = y.reshape(batchSize, self.F[-1] * self.N[-1])
        return self.MLP(y)


class _GatedGCRNNBase(nn.Module):
    def _init_state(self, inFeatures, stateFeatures, inputFilterTaps, stateFilterTaps, stateNonlinearity,
                    outputNonlinearity, dimLayersMLP, GSO, bias, time_gating, spatial_gating, finalNonlinearity,
                    dimNodeSignals, nFilterTaps, nSelectedNodes=None, poolingFunction=None, poolingSize=None, maxN=None):
        S = _as_gso_tensor(GSO)
        self.F_i, self.K_i = inFeatures, inputFilterTaps
        self.F_h, self.K_h = stateFeatures, stateFilterTaps
        self.E, self.N = int(S.shape[0]), int(S.shape[1])
        self.bias = bias
        self.time_gating = time_gating
        self.spatial_gating = spatial_gating
        self.register_buffer('S', S, persistent=False)            # moved by .to(); not in state_dict (as the reference)
        self.sigma1 = stateNonlinearity
        self.stateGCRNN = gml.GGCRNNCell(self.F_i, self.F_h, self.K_i, self.K_h, self.sigma1, self.time_gating,
                                         self.spatial_gating, self.E, self.bias)
        self.stateGCRNN.addGSO(self.S)
        self.dimLayersMLP = dimLayersMLP
        self.sigma2 = outputNonlinearity
        self.sigma3 = finalNonlinearity
        self.F_o = dimNodeSignals
        self.K_o = nFilterTaps
        self.nSelectedNodes = nSelectedNodes
        self.rho = poolingFunction
        self.alpha = poolingSize
        self.maxN = maxN
        self.gnn_head = not (dimNodeSignals is None and nFilterTaps is None)
        if self.gnn_head and nSelectedNodes is None and poolingFunction is not gml.NoPool:      # reference :1571-1586
            raise NotImplementedError('AggregationGNN output heads are not implemented; give nSelectedNodes and poolingFunction=NoPool '
                                      'for a Selection-GNN head, or use the MLP heads (dimNodeSignals=None, nFilterTaps=None)')

    def _selection_head(self, GSO):
        """outputNN of the Selection-GNN branch (reference :1588-1604 / :1823-1839): SelectionGNN + the final nonlinearity."""
        sel = [SelectionGNN(self.F_o, self.K_o, self.bias, self.sigma2, self.nSelectedNodes, self.rho, self.alpha, self.dimLayersMLP, GSO)]
        if self.sigma3 is not None:
            sel.append(self.sigma3())
        return nn.Sequential(*sel)

    def _after_head(self, y):
        """What outputNN holds behind the layer a small-graph launch has evaluated: the finalNonlinearity, where there is one."""
        for layer in self.outputNN[1:]:
            y = layer(y)
        return y


class GatedGCRNNforRegression(_GatedGCRNNBase):
    """State cell + MLP head on every h_t (reference architectures.py:1405-1645).

    forward(x: B x T x F_i x N, h0: B x F_h x N) -> B x T x 1 x (N*out).
    """

    def __init__(self, inFeatures, stateFeatures, inputFilterTaps, stateFilterTaps, stateNonlinearity,
                 outputNonlinearity, dimLayersMLP, GSO, bias, time_gating=True, spatial_gating=None,
                 mlpType='oneMlp', finalNonlinearity=None, dimNodeSignals=None, nFilterTaps=None,
                 nSelectedNodes=None, poolingFunction=None, poolingSize=None, maxN=None):
        super().__init__()
        self._init_state(inFeatures, stateFeatures, inputFilterTaps, stateFilterTaps, stateNonlinearity,
                         outputNonlinearity, dimLayersMLP, GSO, bias, time_gating, spatial_gating,
                         finalNonlinearity, dimNodeSignals, nFilterTaps, nSelectedNodes, poolingFunction, poolingSize, maxN)
        self.mlpType = mlpType
        if self.gnn_head:
            self.outputNN = self._selection_head(self.S)
            return
        dimInputMLP = self.N * self.F_h if mlpType == 'oneMlp' else self.F_h     # reference :1545-1554
        assert mlpType in ('oneMlp', 'multipMlp')
        self.outputNN = _build_mlp(dimInputMLP, self.dimLayersMLP, self.sigma2, self.sigma3, self.bias)

    def forward(self, x, h0):
        batchSize, seqLength = x.shape[0], x.shape[1]
        if self.gnn_head:
            sel = self.outputNN[0]
            if sel.L == 1 and list(sel.F) == [self.F_h, 1] and len(sel.dimLayersMLP) == 0 and sel.GFL[0].weight.dtype == x.dtype:
                # a head of ONE graph-filter layer with one output feature on a small graph: y_t from the hop levels of the state still
                # in the forward launch's LDS, dH_t formed inside the BPTT launch from the head's adjoint -- neither the T states
                # (inference) nor dH (training) are materialised; None: not that path
                gfl, sigma = sel.GFL[0], sel.GFL[1]
                act = _FUSED_ACTIVATIONS.get(type(sigma))
                y = self.stateGCRNN.regress_gnn(x, h0, gfl.weight, gfl.bias, act)      # B x T x 1 x N
                if y is not None:
                    if act is None:
                        y = sigma(y)
                    return self._after_head(y)
            # the Selection-GNN head on all B*T states (reference :1630-1632): H [B][T][F_h][N] is already its [items][F][N] input
            H = self.stateGCRNN(x, h0)
            flatY = self.outputNN(H.reshape(-1, self.F_h, self.N))
            return flatY.reshape(batchSize, seqLength, -1).unsqueeze(2)
        if self.mlpType == 'multipMlp' and not torch.is_grad_enabled() and len(self.outputNN) == 1 and \
                isinstance(self.outputNN[0], nn.Linear) and self.outputNN[0].out_features == 1:
            # inference with the drivers' head (dimLayersMLP = [1]): fused onto the cell's h_t store, H is never materialised
            y = self.stateGCRNN.forward_with_head(x, h0, self.outputNN[0].weight, self.outputNN[0].bias)
            if y is not None:
                return y.to(x.dtype)
        if self.mlpType == 'multipMlp' and torch.is_grad_enabled() and len(self.outputNN) == 1 and \
                isinstance(self.outputNN[0], nn.Linear) and self.outputNN[0].out_features == 1:
            # training with the drivers' head: cell + head as one autograd node whose backward hands the head's gradient to the BPTT
            # chain as (w, dy) -- dH is never materialised; same values and gradients as the two modules below
            y = self.stateGCRNN.train_with_head(x, h0, self.outputNN[0].weight, self.outputNN[0].bias)
            if y is not None:
                return y
        if self.mlpType == 'multipMlp' and len(self.dimLayersMLP) == 1 and isinstance(self.outputNN[0], nn.Linear) and \
                self.outputNN[0].weight.dtype == x.dtype:
            # the drivers' head (dimLayersMLP = [O]) on a small graph: y_t from the state still in the forward launch's LDS, dH_t formed
            # inside the BPTT launch -- neither the T states (inference) nor dH (training) are materialised; None: not that path
            y = self.stateGCRNN.regress(x, h0, self.outputNN[0].weight, self.outputNN[0].bias)      # B x T x O x N
            if y is not None:
                y = y.reshape(batchSize, seqLength, -1).unsqueeze(2)
                return self._after_head(y)
        H = self.stateGCRNN(x, h0)                                  # B x T x F_h x N
        flatH = H.reshape(-1, self.F_h, self.N)
        if self.mlpType == 'multipMlp':
            # one perceptron shared by all nodes (reference :1616-1627 loops over nodes; here one batched GEMM)
            assert self.F_h > 1, "the reference's per-node squeeze() breaks for F_h = 1 (architectures.py:1622)"
            lin = self.outputNN[0] if len(self.outputNN) == 1 and isinstance(self.outputNN[0], nn.Linear) else None
            if lin is not None and ops.node_linear_supported(self.F_h, lin.out_features, flatH.dtype, self.N, lin.weight.dtype):
                # the drivers' head (dimLayersMLP = [1]): one kernel on the user layout, no transposes
                flatY = ops.node_linear(flatH, lin.weight, lin.bias)            # (BT) x out x N
                return flatY.reshape(batchSize, seqLength, -1).unsqueeze(2)
            rows = _to_param_dtype(flatH, self.outputNN).transpose(1, 2).reshape(-1, self.F_h)                  # (BT*N) x F_h
            flatY = _apply_mlp_rows(self.outputNN, rows).reshape(flatH.shape[0], self.N, -1).transpose(1, 2)   # (BT) x out x N
        else:
            flatY = self.outputNN(_to_param_dtype(flatH, self.outputNN).reshape(-1, self.F_h * self.N))
        return flatY.reshape(batchSize, seqLength, -1).unsqueeze(2)


class GatedGCRNNforClassification(_GatedGCRNNBase):
    """State cell + MLP on the last state only (reference architectures.py:1647-1859). Returns B x C logits."""

    def __init__(self, inFeatures, stateFeatures, inputFilterTaps, stateFilterTaps, stateNonlinearity,
                 outputNonlinearity, dimLayersMLP, GSO, bias, time_gating=True, spatial_gating=None,
                 finalNonlinearity=None, dimNodeSignals=None, nFilterTaps=None,
                 nSelectedNodes=None, poolingFunction=None, poolingSize=None, maxN=None):
        super().__init__()
        self._init_state(inFeatures, stateFeatures, inputFilterTaps, stateFilterTaps, stateNonlinearity,
                         outputNonlinearity, dimLayersMLP, GSO, bias, time_gating, spatial_gating,
                         finalNonlinearity, dimNodeSignals, nFilterTaps, nSelectedNodes, poolingFunction, poolingSize, maxN)
        if self.gnn_head:
            self.outputNN = self._selection_head(self.S)
        else:
            self.outputNN = _build_mlp(self.N * self.F_h, self.dimLayersMLP, self.sigma2, self.sigma3, self.bias)

    def forward(self, x, h0):
        if not self.gnn_head and len(self.dimLayersMLP) == 1 and isinstance(self.outputNN[0], nn.Linear) and \
                self.outputNN[0].weight.dtype == x.dtype:
            # the drivers' head (dimLayersMLP = [C]) on a small graph: recurrence and read-out in one launch, BPTT started from dlogits
            # inside its launch -- neither the T states (inference) nor dH (training) are materialised; None: not that path
            y = self.stateGCRNN.classify(x, h0, self.outputNN[0].weight, self.outputNN[0].bias)
            if y is not None:
                return self._after_head(y)
        if self.gnn_head:
            sel = self.outputNN[0]
            if sel.L == 1 and list(sel.F) == [self.F_h, 1] and len(sel.dimLayersMLP) == 1 and len(sel.MLP) == 1 and \
                    type(sel.GFL[1]) in _FUSED_ACTIVATIONS and sel.GFL[0].weight.dtype == x.dtype:
                # a head of ONE graph-filter layer with one output feature and one Linear behind a fused activation, on a small graph: the
                # last state's hop levels, the filter, the activation and the read-out run in the forward launch, the BPTT launch starts
                # from dlogits -- neither the T states (inference) nor dH (training) are materialised; None: not that path. The
                # parameters are read at every call
                gfl, lin = sel.GFL[0], sel.MLP[0]
                y = self.stateGCRNN.classify_gnn(x, h0, gfl.weight, gfl.bias, _FUSED_ACTIVATIONS[type(sel.GFL[1])], lin.weight, lin.bias)
                if y is not None:
                    return self._after_head(y)
        H = self.stateGCRNN(x, h0, last_only=not torch.is_grad_enabled())     # inference: only the last state is materialised
        h = H.select(1, -1)                                          # reference :1844
        if self.gnn_head:
            return self.outputNN(h)                                  # reference :1848-1849
        return self.outputNN(_to_param_dtype(h, self.outputNN).reshape(-1, self.F_h * self.N))


class _RNNParameters(nn.Module):
    """The parameters of the reference's torch.nn.RNN(D, F_h, num_layers=1, nonlinearity, bias, batch_first=True), under the same
    names (`weight_ih_l0`, `weight_hh_l0`, `bias_ih_l0`, `bias_hh_l0`) and drawn in the same order with the same
    uniform(-1/sqrt(F_h), 1/sqrt(F_h)), so that seeded models start from the reference's values. The recurrence itself is
    ops.rnn_sequence (gcrnn_rnn.hip); torch.nn.RNN is not instantiated."""

    def __init__(self, input_size, hidden_size, nonlinearity='tanh', bias=True):
        super().__init__()
        if nonlinearity not in ('tanh', 'relu'):                   # torch.nn.RNN's check, before any parameter exists
            raise ValueError("Unknown nonlinearity '%s'. Select from 'tanh' or 'relu'." % (nonlinearity,))
        if not isinstance(hidden_size, int):
            raise TypeError('hidden_size should be of type int, got: %s' % type(hidden_size).__name__)
        if hidden_size <= 0:
            raise ValueError('hidden_size must be greater than zero')
        self.input_size, self.hidden_size, self.nonlinearity, self.bias = input_size, hidden_size, nonlinearity, bias
        self.weight_ih_l0 = nn.Parameter(torch.empty(hidden_size, input_size))
        self.weight_hh_l0 = nn.Parameter(torch.empty(hidden_size, hidden_size))
        if bias:
            self.bias_ih_l0 = nn.Parameter(torch.empty(hidden_size))
            self.bias_hh_l0 = nn.Parameter(torch.empty(hidden_size))
        else:
            self.bias_ih_l0 = self.bias_hh_l0 = None
        stdv = 1.0 / np.sqrt(hidden_size)
        for p in self.parameters():                                  # torch.nn.RNN.reset_parameters
            nn.init.uniform_(p, -stdv, stdv)

    def forward(self, x, h0):
        """x: B x T x D, h0: B x F_h -> H: B x T x F_h."""
        return ops.rnn_sequence(x, h0, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0, self.nonlinearity)


class _RNNBase(nn.Module):
    def _init_rnn(self, inFeatures, stateFeatures, stateNonlinearity, dimLayersMLP, outputNonlinearity, GSO, bias,
                  finalNonlinearity, outMult):
        S = _as_gso_tensor(GSO)
        self.F_i = inFeatures
        self.F_h = stateFeatures
        self.E = int(S.shape[0])
        self.N = int(S.shape[1])
        self.bias = bias
        self.register_buffer('S', S, persistent=False)            # moved by .to(); not in state_dict (as the reference)
        self.sigma1 = stateNonlinearity
        self.RNN = _RNNParameters(self.N * self.F_i, self.F_h, nonlinearity=self.sigma1, bias=self.bias)
        self.dimLayersMLP = dimLayersMLP
        self.sigma2 = outputNonlinearity
        self.sigma3 = finalNonlinearity
        fc = []                                                   # reference :1952-1968 / :2102-2118; the last layer's width * outMult
        if len(dimLayersMLP) > 0:
            if len(dimLayersMLP) != 1:
                fc.append(nn.Linear(self.F_h, dimLayersMLP[0], bias=self.bias))
                for l in range(len(dimLayersMLP) - 1):
                    fc.append(self.sigma2())
                    last = l == len(dimLayersMLP) - 2
                    fc.append(nn.Linear(dimLayersMLP[l], dimLayersMLP[l + 1] * (outMult if last else 1), bias=self.bias))
            else:
                fc.append(nn.Linear(self.F_h, dimLayersMLP[0] * outMult, bias=self.bias))
        if self.sigma3 is not None:
            fc.append(self.sigma3())
        self.outputNN = nn.Sequential(*fc)

    def _states(self, x, h0):
        batchSize, seqLength = x.shape[0], x.shape[1]
        return self.RNN(x.reshape(batchSize, seqLength, -1), h0.reshape(batchSize, -1))      # B x T x F_h


class RNNforRegression(_RNNBase):
    """The drivers' RNN baseline for regression (reference architectures.py:1861-2004): a one-layer RNN on the flattened graph signal
    (input index f*N + n) and an MLP on every state. Same signature, state_dict keys (`RNN.weight_ih_l0`, ..., `outputNN.<i>.*`) and
    seeded initialisation. The recurrence runs on the HIP kernels of ops.rnn_sequence; the MLP is nn.Linear.

    forward(x: B x T x F_i x N, h0: B x F_h, c0: ignored) -> B x T x out x N.
    """

    def __init__(self, inFeatures, stateFeatures, stateNonlinearity, dimLayersMLP, outputNonlinearity, GSO, bias,
                 finalNonlinearity=None):
        super().__init__()
        self._init_rnn(inFeatures, stateFeatures, stateNonlinearity, dimLayersMLP, outputNonlinearity, GSO, bias, finalNonlinearity,
                       _as_gso_tensor(GSO).shape[1])

    def forward(self, x, h0, c0):
        batchSize, seqLength = x.shape[0], x.shape[1]
        H = self._states(x, h0)
        flatY = self.outputNN(_to_param_dtype(H.reshape(batchSize * seqLength, self.F_h), self.outputNN))
        return flatY.view(batchSize, seqLength, -1, self.N)


class RNNforClassification(_RNNBase):
    """The drivers' RNN baseline for classification (reference architectures.py:2006-2149): the MLP on the last state only.

    forward(x: B x T x F_i x N, h0: B x F_h, c0: ignored) -> B x dimLayersMLP[-1].
    """

    def __init__(self, inFeatures, stateFeatures, stateNonlinearity, dimLayersMLP, outputNonlinearity, GSO, bias,
                 finalNonlinearity=None):
        super().__init__()
        self._init_rnn(inFeatures, stateFeatures, stateNonlinearity, dimLayersMLP, outputNonlinearity, GSO, bias, finalNonlinearity, 1)

    def forward(self, x, h0, c0):
        H = self._states(x, h0)
        return self.outputNN(_to_param_dtype(H.select(1, -1), self.outputNN))
