"""Training of cell + output head Linear(F -> 1) shared by all nodes without dH: the wide BPTT chain takes the head's gradient as its factors
(w_head, dy) and makes bf16(w_head[f] dy[n]) in its epilogue (csrc/gcrnn_fused_seq32.h MODE 2 with VAR bit 4,
gcrnn_fused_backward_data_wide_head_bf16; ops.fused_backward_data_head, ops.fused_cell_head_train, GGCRNNCell.train_with_head). That product
rounded to bf16 is what the head's backward kernel stores into dH on the two-module path, so everything here is pinned to that path BIT FOR BIT
(there is no tolerance to choose); one test ties the shared result to the same model in fp32."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_wide import _uniform_cell

_ENVS = ('GCRNN_SEQ32', 'GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ_KERNEL', 'GCRNN_SEQ32_SPLIT', 'GCRNN_NO_WIDE_CHAIN', 'GCRNN_NO_HEAD_CHAIN')


# ------------------------------------------------------------------------------------------ CPU: ABI, query, argument checks
def test_head_chain_entry_points_are_declared_and_the_query_answers_without_a_device(monkeypatch):
    import os
    from conftest import ROOT
    from gated_gcrnns_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    for n in ('gcrnn_fused_backward_data_wide_head_supported', 'gcrnn_fused_backward_data_wide_head_bf16'):
        assert n in _lib.EXPORTS and (n + '(') in hdr
    for e in _ENVS:
        monkeypatch.delenv(e, raising=False)
    q = _lib.lib.gcrnn_fused_backward_data_wide_head_supported
    assert q(256, 32, 1000, 64, 5, 732, 0.1, 1) == 1
    assert q(256, 32, 1000, 64, 5, 732, 0.0, 1) == 0          # weighted graph
    assert q(256, 32, 1000, 64, 5, 732, 0.1, 3) == 0          # rank-1-weighted graph
    assert q(256, 32, 1000, 48, 5, 732, 0.1, 1) == 0          # F = 48
    assert q(256, 32, 1000, 64, 5, 4000, 0.1, 1) == 0         # LDS
    assert q(100, 32, 1000, 64, 5, 732, 0.1, 1) == 0          # a split batch: one launch per step
    assert q(4096, 1024, 1000, 64, 5, 732, 0.1, 1) == 0       # B*T*N*2 past 31 bits
    # ... and it never says yes where the chain it is a variant of says no
    assert _lib.lib.gcrnn_fused_backward_data_wide_supported(256, 32, 1000, 64, 5, 732, 0.1, 1, 0) == 1


def _entry_args(ptr, dy, w, B=256, T=4, N=1000, F=64, K=5, entries=732):
    return (dy, w, ptr, ptr, None, ptr, ptr, ptr, ptr, entries, B, T, N, F, K, None, None, None, None)


def test_head_chain_entry_point_validates_before_any_launch(monkeypatch):
    """CPU: every argument check sits in front of the first launch (the pointers are never dereferenced on the host)."""
    from gated_gcrnns_amd import _lib
    for e in _ENVS:
        monkeypatch.delenv(e, raising=False)
    buf = (C.c_char * 96)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)
    f = _lib.lib.gcrnn_fused_backward_data_wide_head_bf16
    assert f(*_entry_args(ptr, None, ptr)) == 3                      # GCRNN_ERR_NULL_POINTER: no dy
    assert f(*_entry_args(ptr, ptr, None)) == 3                      # ... no head weights
    assert f(*_entry_args(ptr, ptr, ptr, B=100)) == 4                # GCRNN_ERR_UNSUPPORTED: a split batch
    assert f(*_entry_args(ptr, ptr, ptr, F=48)) == 4                 # ... no such instantiation
    assert f(*_entry_args(ptr, ptr, ptr, B=4096, T=1024)) == 2       # GCRNN_ERR_BAD_SHAPE: dy past the 32-bit offsets
    assert f(*_entry_args(ptr, C.c_void_p(ptr.value + 1), ptr)) == 2      # dy is an array of 2-byte elements


# ------------------------------------------------------------------------------------------ GPU A: the chain against the parent's chain
CHAIN_SHAPES = [(1000, 64, 5, 4, 5, False, 'f32'), (1000, 64, 5, 3, 4, True, 'f32'),
                (400, 32, 3, 6, 4, True, 'f32'),            # K < 4: the requests sit in front of hop 1
                (1000, 64, 2, 2, 3, False, 'f32'),
                (1000, 64, 4, 3, 1, True, 'f32'),           # T = 1: only the seed and the final step run
                (1008, 64, 5, 130, 3, False, 'f32'),
                (251, 32, 3, 5, 3, True, 'f32'),            # odd N: rows of dy start 2-byte aligned only, rows 251..255 of the last tile read 0
                (1000, 64, 5, 3, 4, True, 'bf16w')]         # bf16-valued head weights


@pytest.mark.gpu
@pytest.mark.parametrize('N,F,K,B,T,gated,wkind', CHAIN_SHAPES)
def test_head_chain_equals_the_chain_on_the_materialised_gradient(N, F, K, B, T, gated, wkind, monkeypatch):
    """ops.fused_backward_data_head(dy, w) against ops.fused_backward_data on dH = bf16(w (x) dy) laid out by ops.fused_pack_upstream (the
    existing code, unchanged): dpre of every step, d h0 and d gf are EQUAL."""
    from gated_gcrnns_amd import ops
    dev = torch.device('cuda:0')
    cell, rng, S = _uniform_cell(N, F, F, K, 29)
    cell = cell.to(dev)
    dy = torch.tensor(rng.standard_normal((B, T, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    w = torch.tensor(rng.uniform(-1.0, 1.0, F), dtype=torch.float32, device=dev)
    if wkind == 'bf16w':
        w = w.to(torch.bfloat16).float()
    H = torch.tanh(torch.tensor(rng.standard_normal((B, T, F, N)), dtype=torch.float32, device=dev)).to(torch.bfloat16)
    h0 = torch.tensor(0.3 * rng.standard_normal((B, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    gf = torch.tensor(rng.uniform(0.2, 0.9, (T, B)), dtype=torch.float32, device=dev) if gated else None
    hs = ops.to_sequence_major(H, cell.graph)
    h0s = ops.to_sequence_major(h0.view(B, 1, F, N), cell.graph)
    wB = cell.weight_B.detach().float()
    bias = cell.bias.detach().float()
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    for e in ('GCRNN_NO_WIDE_CHAIN', 'GCRNN_NO_INLINE_PACK'):
        monkeypatch.delenv(e, raising=False)
    assert ops.fused_backward_data_head_plan(cell.graph, B, T, N, F, K) is not None
    dH = (dy.float().unsqueeze(2) * w.view(1, 1, F, 1)).to(torch.bfloat16)
    dHs, dHu = ops.fused_pack_upstream(dH, cell.graph, K)
    if gated:
        want = ops.fused_backward_data(dHs, hs, wB, cell.graph, want_dh0=True, gf=gf, h0s=h0s, bias=bias, dH_user=dHu)
        got = ops.fused_backward_data_head(dy, w, hs, wB, cell.graph, want_dh0=True, gf=gf, h0s=h0s, bias=bias)
    else:
        want = ops.fused_backward_data(dHs, hs, wB, cell.graph, want_dh0=True, dH_user=dHu)
        got = ops.fused_backward_data_head(dy, w, hs, wB, cell.graph, want_dh0=True)
    torch.cuda.synchronize()
    assert len(got) == len(want) == (3 if gated else 2)
    for t in range(T):
        assert float(want[0][t].float().std()) > 0 and float(got[0][t].float().std()) > 0, t
    for name, a_, b_ in zip(('dpre', 'dh0', 'dgf'), got, want):
        ne = int((a_ != b_).sum())
        print('%s: %d of %d elements differ' % (name, ne, a_.numel()))
        assert torch.equal(a_, b_), (name, ne)


# ------------------------------------------------------------------------------------------ GPU B-E: the model
def _graph(N, seed, weighted=False):
    rng = np.random.default_rng(seed)
    W = (rng.random((N, N)) < 10.0 / N).astype(np.float64)
    W = np.triu(W, 1); W = W + W.T
    if weighted:
        R = np.triu(rng.uniform(0.5, 1.0, (N, N)), 1)
        W = W * (R + R.T)
    return W / np.max(np.abs(np.linalg.eigvalsh(W))), rng


def _model(dev, S, F, K, tg=False, layers=(1,), mlp='multipMlp', sg=None):
    import gated_gcrnns_amd.Modules.architectures as archit
    torch.manual_seed(29)
    m = archit.GatedGCRNNforRegression(F, F, K, K, torch.tanh, torch.nn.ReLU, list(layers), S, True, time_gating=tg, spatial_gating=sg, mlpType=mlp)
    return m.to(torch.bfloat16).to(torch.float32).to(dev)             # bf16-representable values, fp32 storage


class _Spies(object):
    """Counts the calls of the new entry and of ops.fused_pack_upstream, and records the `dh` argument of the head's backward kernel."""

    def __init__(self, monkeypatch):
        from gated_gcrnns_amd import _lib, ops
        self.chain, self.pack, self.dh = [], [], []
        o1, o2, o3 = _lib.lib.gcrnn_fused_backward_data_wide_head_bf16, _lib.lib.gcrnn_node_linear_bf16_backward, ops.fused_pack_upstream
        monkeypatch.setattr(_lib.lib, 'gcrnn_fused_backward_data_wide_head_bf16', lambda *a: (self.chain.append(1), o1(*a))[1], raising=False)
        monkeypatch.setattr(_lib.lib, 'gcrnn_node_linear_bf16_backward', lambda *a: (self.dh.append(a[4]), o2(*a))[1], raising=False)
        monkeypatch.setattr(ops, 'fused_pack_upstream', lambda *a, **k: (self.pack.append(1), o3(*a, **k))[1])

    def reset(self):
        del self.chain[:], self.pack[:], self.dh[:]


def _step(m, X, h0, target, switch_off, monkeypatch):
    """One forward + L1 loss + backward of the model; returns (y, loss, {name: grad}, X.grad, h0.grad)."""
    import gated_gcrnns_amd.Utils.miscTools as misc
    if switch_off:
        monkeypatch.setenv('GCRNN_NO_HEAD_CHAIN', '1')
    else:
        monkeypatch.delenv('GCRNN_NO_HEAD_CHAIN', raising=False)
    m.zero_grad(set_to_none=True)
    X.grad = h0.grad = None
    y = m(X, h0)
    loss = misc.batchTimeL1Loss(y, target)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in m.named_parameters()}
    return y.detach().clone(), loss.detach().clone(), grads, (X.grad.clone() if X.grad is not None else None), (h0.grad.clone() if h0.grad is not None else None)


def _same(a, b):
    assert tuple(a[0].shape) == tuple(b[0].shape) and a[0].dtype == b[0].dtype
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert sorted(a[2]) == sorted(b[2])
    for n in a[2]:
        assert (a[2][n] is None) == (b[2][n] is None), n
        if a[2][n] is not None:
            assert torch.equal(a[2][n], b[2][n]), (n, float((a[2][n] - b[2][n]).abs().max()))
    for i in (3, 4):
        assert (a[i] is None) == (b[i] is None)
        if a[i] is not None:
            assert torch.equal(a[i], b[i]), i


MODEL = dict(N=200, F=32, K=3, B=6, T=4)


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
def test_regression_model_trains_through_the_head_chain_with_the_two_module_paths_bits(tg, monkeypatch):
    N, F, K, B, T = (MODEL[k] for k in ('N', 'F', 'K', 'B', 'T'))
    dev = torch.device('cuda:0')
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    S, rng = _graph(N, 61)
    m = _model(dev, S, F, K, tg)
    Xf = torch.tensor(rng.standard_normal((B, T, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    hf = torch.zeros((B, F, N), dtype=torch.bfloat16, device=dev)
    # fp32 reference: the same model on fp32 tensors. Two properties of the L1 loss decide what a comparison with fp32 can show, and the
    # target is laid out for both from the REFERENCE's own output, before the code under test runs: (1) the loss has a kink at y == target, where
    # a last-bit difference of y flips a gradient's sign -- the target stays 0.5 .. 1.5 away from y_ref; (2) every element's gradient is
    # +-1 / count, and a scalar parameter (a time gate's read-out bias) sums all of them -- with random signs that sum cancels to a few
    # 1e-6 and its relative error says nothing (measured so: 0.12 on MLP_in.0.bias with every tensor-valued gradient within 2e-2). The offset
    # therefore points along sign(y_ref): locally the loss is const - mean|y|, whose gate gradients are sums of like terms.
    ref = _model(dev, S, F, K, tg)
    yr = ref(Xf.float(), hf.float())
    sgn = torch.where(yr.detach() >= 0, 1.0, -1.0)
    off = sgn * torch.tensor(rng.uniform(0.5, 1.5, tuple(yr.shape)), dtype=torch.float32, device=dev)
    target = (yr.detach() + off).to(torch.bfloat16)
    import gated_gcrnns_amd.Utils.miscTools as misc
    misc.batchTimeL1Loss(yr, target.float()).backward()
    spies = _Spies(monkeypatch)
    new = _step(m, Xf, hf, target, False, monkeypatch)
    assert len(spies.chain) == 1 and len(spies.pack) == 0              # once per backward; no dH to lay out
    assert len(spies.dh) == 1 and spies.dh[0] is None                  # the head's kernel stores no dH
    assert tuple(new[0].shape) == (B, T, 1, N) and new[0].dtype == torch.bfloat16
    spies.reset()
    old = _step(m, Xf, hf, target, True, monkeypatch)
    assert len(spies.chain) == 0 and len(spies.pack) == 1 and spies.dh[0] is not None
    _same(new, old)
    for n in ('outputNN.0.weight', 'outputNN.0.bias', 'stateGCRNN.weight_A', 'stateGCRNN.weight_B', 'stateGCRNN.bias'):
        assert new[2][n] is not None and float(new[2][n].abs().max()) > 0, n
    # the shared result against fp32 (the gates of test_fused_cell_inside_the_models_bf16_activations_fp32_master_weights)
    yr = yr.detach()
    sc = float(yr.abs().max())
    ey = float((new[0].float() - yr).abs().max())
    print('y vs fp32: %.3e of the scale (gate 3e-2)' % (ey / sc))
    assert ey <= 3e-2 * sc, ey / sc
    for n, p in ref.named_parameters():
        if p.grad is None:
            assert new[2][n] is None, n
            continue
        g, gr = new[2][n].float(), p.grad
        s = float(gr.abs().max())
        if s == 0.0:                                   # h0 = 0: the gate cells' state taps get exactly no gradient, in both
            assert float(g.abs().max()) == 0.0, n
            continue
        e = (g - gr).abs()
        print('%s: max %.3e mean %.3e of its max (gates 5e-2, 1e-2)' % (n, float(e.max()) / s, float(e.mean()) / s))
        assert float(e.max()) <= 5e-2 * s and (e.numel() < 16 or float(e.mean()) <= 1e-2 * s), (n, float(e.max()) / s, float(e.mean()) / s)


@pytest.mark.gpu
def test_head_chain_gives_the_input_and_initial_state_gradients(monkeypatch):
    N, F, K, B, T = (MODEL[k] for k in ('N', 'F', 'K', 'B', 'T'))
    dev = torch.device('cuda:0')
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    S, rng = _graph(N, 63)
    m = _model(dev, S, F, K, False)
    X = torch.tensor(rng.standard_normal((B, T, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16).requires_grad_(True)
    h0 = torch.tensor(0.3 * rng.standard_normal((B, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16).requires_grad_(True)
    target = torch.tensor(rng.standard_normal((B, T, 1, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    spies = _Spies(monkeypatch)
    new = _step(m, X, h0, target, False, monkeypatch)
    assert len(spies.chain) == 1 and len(spies.pack) == 0
    old = _step(m, X, h0, target, True, monkeypatch)
    assert len(spies.chain) == 1
    assert new[3] is not None and new[4] is not None and float(new[3].float().std()) > 0 and float(new[4].float().std()) > 0
    _same(new, old)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['weighted', 'two_outputs', 'oneMlp', 'node_gated'])
def test_other_models_keep_the_two_module_path(kind, monkeypatch):
    N, F, K, B, T = (MODEL[k] for k in ('N', 'F', 'K', 'B', 'T'))
    dev = torch.device('cuda:0')
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    S, rng = _graph(N, 65, weighted=(kind == 'weighted'))
    m = _model(dev, S, F, K, False, layers=(2,) if kind == 'two_outputs' else (1,), mlp='oneMlp' if kind == 'oneMlp' else 'multipMlp',
               sg='node' if kind == 'node_gated' else None)
    X = torch.tensor(rng.standard_normal((B, T, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    h0 = torch.zeros((B, F, N), dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        shape = tuple(m(X, h0).shape)
    target = torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=dev).to(torch.bfloat16)
    spies = _Spies(monkeypatch)
    new = _step(m, X, h0, target, False, monkeypatch)
    old = _step(m, X, h0, target, True, monkeypatch)
    assert len(spies.chain) == 0
    _same(new, old)


@pytest.mark.gpu
def test_head_chain_training_step_is_capturable(monkeypatch):
    """train_rnn.GraphedTrainStep of the model (zero_grad, forward, L1 loss, BPTT, FlatAdam as ONE captured graph): the capture succeeds -- the
    new entry allocates nothing of its own and does not synchronise -- and every replay gives the loss of the same step run eagerly, bit for
    bit, with the parameters following."""
    from gated_gcrnns_amd.Modules.train_rnn import train_step, GraphedTrainStep
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    from gated_gcrnns_amd.optim import FlatAdam
    N, F, K, B, T = (MODEL[k] for k in ('N', 'F', 'K', 'B', 'T'))
    dev = torch.device('cuda:0')
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    monkeypatch.delenv('GCRNN_NO_HEAD_CHAIN', raising=False)
    S, rng = _graph(N, 67)
    ms = [_model(dev, S, F, K, True), _model(dev, S, F, K, True)]      # (one seed: equal parameters)
    X = torch.tensor(rng.standard_normal((B, T, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    target = torch.tensor(rng.standard_normal((B, T, 1, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    spies = _Spies(monkeypatch)
    opt_e, opt_g = FlatAdam(ms[0].parameters(), lr=1e-3), FlatAdam(ms[1].parameters(), lr=1e-3)
    stepper = GraphedTrainStep(ms[1], batchTimeL1Loss, opt_g, X, target, F)      # three eager warm-up steps, then the capture
    assert stepper.captured and len(spies.chain) == 4 and len(spies.pack) == 0
    for _ in range(3):
        train_step(ms[0], batchTimeL1Loss, opt_e, X, target, F)
    spies.reset()
    for it in range(3):
        le, _ = train_step(ms[0], batchTimeL1Loss, opt_e, X, target, F)
        lg, _ = stepper(X, target)
        assert float(le) == float(lg), it
    assert len(spies.chain) == 3                                       # (the eager twin's; a replay calls nothing on the host)
    for p, q in zip(ms[0].parameters(), ms[1].parameters()):
        assert torch.equal(p, q)
