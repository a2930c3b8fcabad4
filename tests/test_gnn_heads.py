"""GPU: the GNN output heads on the graph-filter layer kernel (gcrnn_readout.hip) -- the G15 fixtures of the reference's autograd,
the kernel against a numpy fp64 filter at N = 1000, determinism of the weight gradients, the kernel actually taken (composed
fallback made to raise), one bf16 training step through the fused cell, and the reference's Adam trace."""
import os
import unittest.mock as mock

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import gated_gcrnns_amd.Utils.graphML as gml
import gated_gcrnns_amd.Modules.architectures as archit
from gated_gcrnns_amd import ops
from gated_gcrnns_amd.graph import GraphOperator

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ACTS = {None: lambda v: v, 'relu': lambda v: np.maximum(v, 0.0), 'tanh': np.tanh, 'sigmoid': lambda v: 1.0 / (1.0 + np.exp(-v))}
DACT = {None: lambda y: np.ones_like(y), 'relu': lambda y: (y > 0).astype(y.dtype), 'tanh': lambda y: 1.0 - y * y,
        'sigmoid': lambda y: y * (1.0 - y)}


def sbm_uniform(N, seed):
    rng = np.random.default_rng(seed)
    lab = np.arange(N) * 5 // N
    P = np.where(lab[:, None] == lab[None, :], 0.04, 0.0025)
    U = np.triu(rng.random((N, N)) < P, 1)
    W = (U + U.T).astype(np.float64)
    return (W / np.max(np.linalg.eigvalsh(W))).reshape(1, N, N)


def random_directed(N, density, seed):
    rng = np.random.default_rng(seed)
    S = (rng.random((N, N)) < density) * rng.uniform(0.2, 1.0, (N, N))
    return (S / np.max(np.abs(np.linalg.eigvals(S)))).reshape(1, N, N)


def np_filter(x, w, b, S, act):
    """y[i][o][n] = act(sum_k w[o][0][k] . (x_i S^k) + b[o]) in fp64; returns y and the z_k."""
    K = w.shape[2]
    z = [x]
    for _ in range(1, K):
        z.append(z[-1] @ S)
    pre = sum(np.einsum('of,ifn->ion', w[:, 0, k], z[k]) for k in range(K)) + b.reshape(1, -1, 1)
    return ACTS[act](pre), z


def np_filter_backward(x, w, y, dy, S, act):
    K = w.shape[2]
    g = dy * DACT[act](y)
    u = [g]
    for _ in range(1, K):
        u.append(u[-1] @ S.T)
    dx = sum(np.einsum('of,ion->ifn', w[:, 0, k], u[k]) for k in range(K))
    dw = np.stack([np.einsum('ifn,ion->of', x, u[k]) for k in range(K)], axis=1)[:, None]
    return dx, dw, g.sum(axis=(0, 2)).reshape(-1, 1)


def _model(name, g):
    if name.startswith('g15_sel_quake'):
        return archit.SelectionGNN([20, 21], [4], True, torch.nn.ReLU, [59], gml.NoPool, [1], [11], g['S'][0])
    if name.startswith('g15_sel_kstep'):
        return archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.ReLU, [50, 50], gml.NoPool, [1, 1], [], g['S'][0])
    if name.startswith('g15_cls'):
        return archit.GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [11], g['S'][0], True, name.endswith('time'),
                                                  None, finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[20, 1], nFilterTaps=[4],
                                                  nSelectedNodes=[59], poolingFunction=gml.NoPool, poolingSize=[1])
    F, K = [int(v) for v in g['F']], [int(v) for v in g['K']]
    return archit.GatedGCRNNforRegression(1, 20, 2, 2, torch.tanh, torch.nn.ReLU, [], g['S'][0], True, name.endswith('time'), None,
                                          'oneMlp', torch.nn.ReLU, F, K, [50] * len(K), gml.NoPool, [1] * len(K))


FIXTURES = ['g15_sel_quake', 'g15_sel_kstep', 'g15_cls_gcrnngnn_none', 'g15_cls_gcrnngnn_time', 'g15_reg_gcrnngnn_none',
            'g15_reg_gcrnngnn_time', 'g15_reg_gcrnngnn_deep']


@pytest.mark.parametrize('dt,tol', [(torch.float64, 1e-11), (torch.float32, 1e-5)])
@pytest.mark.parametrize('name', FIXTURES)
def test_g15_fixture_forward_and_gradients(name, dt, tol, monkeypatch):
    g = load_golden(name)
    m = _model(name, g).double()                         # (fp64 parameters first: the fixture's values load exactly)
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    m = m.to(DEV).to(dt)

    def no_fallback(*a, **k):
        raise AssertionError('composed fallback taken')
    monkeypatch.setattr(ops, '_graph_filter_layer_composed', no_fallback)
    ins = [torch.tensor(g['x'], dtype=dt, device=DEV, requires_grad=True)]
    if 'h0' in g:
        ins.append(torch.tensor(g['h0'], dtype=dt, device=DEV, requires_grad=True))
    y = m(*ins)
    (y * torch.tensor(g['R'], dtype=dt, device=DEV)).sum().backward()

    def close(a, ref, what, tol=tol):
        a = a.detach().double().cpu().numpy()
        scale = max(1.0, float(np.max(np.abs(ref))))
        err = float(np.max(np.abs(a - ref))) / scale
        assert err <= tol, '%s %s: rel err %g' % (name, what, err)
    # the head (its output and parameters) at 1e-5 in fp32; gradients that went back through the fp32 recurrence (T = 6..20 steps
    # of BPTT on the cell's own fp32 kernels, held at 2e-5 by the G11 fixtures over shorter chains) at 1e-4
    cell_tol = tol if dt == torch.float64 else 1e-4
    close(y, g['y'], 'y')
    for k, p in m.named_parameters():
        if k in g['grads']:
            close(p.grad, g['grads'][k], k, cell_tol if k.startswith('stateGCRNN.') else tol)
    close(ins[0].grad, g['grad_x'], 'x', cell_tol if len(ins) > 1 else tol)
    if len(ins) > 1:
        close(ins[1].grad, g['grad_h0'], 'h0', cell_tol)


@pytest.mark.parametrize('graph_kind', ['uniform', 'directed'])
@pytest.mark.parametrize('Fout,K', [(1, 1), (1, 2), (1, 5), (4, 1), (4, 2), (4, 5)])
def test_kernel_matches_numpy_filter_bf16_n1000(graph_kind, Fout, K):
    N, Fin, items = 1000, 64, 6
    S = sbm_uniform(N, 3) if graph_kind == 'uniform' else random_directed(N, 0.01, 31)
    graph = GraphOperator(S, device=DEV)
    rng = np.random.default_rng(Fout * 10 + K)
    xb = torch.tensor(rng.standard_normal((items, Fin, N)), dtype=torch.float32).to(torch.bfloat16)
    x64 = xb.double().numpy()
    w = rng.uniform(-1, 1, (Fout, 1, K, Fin)) / np.sqrt(Fin * K)
    b = rng.uniform(-0.5, 0.5, (Fout, 1))
    w32, b32 = w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    S32 = S[0].astype(np.float32).astype(np.float64)
    assert ops.graph_filter_layer_supported(torch.bfloat16, torch.float32, graph, Fin, Fout, K)
    for act in (None, 'relu', 'tanh', 'sigmoid'):
        xd = xb.to(DEV).requires_grad_(True)
        wd = torch.tensor(w32, dtype=torch.float32, device=DEV, requires_grad=True)
        bd = torch.tensor(b32, dtype=torch.float32, device=DEV, requires_grad=True)
        y = ops.graph_filter_layer(xd, wd, bd, graph, act)
        assert y.dtype == torch.float32
        yref, _ = np_filter(x64, w32, b32, S32, act)
        assert np.max(np.abs(y.detach().double().cpu().numpy() - yref)) <= 1e-4 * max(1.0, np.max(np.abs(yref))), act
        dy = rng.standard_normal(y.shape)
        y.backward(torch.tensor(dy, dtype=torch.float32, device=DEV))
        dx, dw, db = np_filter_backward(x64, w32, y.detach().double().cpu().numpy(), dy, S32, act)
        assert xd.grad.dtype == torch.bfloat16
        assert np.max(np.abs(xd.grad.double().cpu().numpy() - dx)) <= 1e-2 * max(1.0, np.max(np.abs(dx))), act
        assert np.max(np.abs(wd.grad.double().cpu().numpy() - dw)) <= 1e-4 * max(1.0, np.max(np.abs(dw))), act
        assert np.max(np.abs(bd.grad.double().cpu().numpy() - db)) <= 1e-4 * max(1.0, np.max(np.abs(db))), act


def test_weight_gradients_are_bit_identical_between_runs():
    N, Fin, Fout, K, items = 1000, 64, 1, 5, 300
    graph = GraphOperator(random_directed(N, 0.01, 5), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn((items, Fin, N), generator=gen, device=DEV).to(torch.bfloat16)
    w = (0.1 * torch.randn((Fout, 1, K, Fin), generator=gen, device=DEV)).requires_grad_(True)
    b = torch.zeros((Fout, 1), device=DEV, requires_grad=True)
    dy = torch.randn((items, Fout, N), generator=gen, device=DEV)
    outs = []
    for _ in range(2):
        w.grad = b.grad = None
        ops.graph_filter_layer(x, w, b, graph, 'tanh').backward(dy)
        outs.append((w.grad.clone(), b.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_driver_and_flagship_shapes_run_on_the_kernel(monkeypatch):
    def no_fallback(*a, **k):
        raise AssertionError('composed fallback taken')
    monkeypatch.setattr(ops, '_graph_filter_layer_composed', no_fallback)
    S59 = np.load(os.path.join(GOLDEN, 'adj59.npy'))
    S59 = S59 / np.max(np.abs(np.linalg.eigvals(S59)))
    torch.manual_seed(0)
    sel = archit.SelectionGNN([20, 21], [4], True, torch.nn.ReLU, [59], gml.NoPool, [1], [11], S59).to(DEV)
    sel(torch.randn(5, 20, 59, device=DEV)).sum().backward()
    S50 = sbm_uniform(50, 1)[0]
    sel = archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.ReLU, [50, 50], gml.NoPool, [1, 1], [], S50).to(DEV)
    sel(torch.randn(5, 1, 50, device=DEV)).sum().backward()
    graph = GraphOperator(sbm_uniform(1000, 0), device=DEV)
    for Fh, K in ((20, 4), (32, 5), (64, 5)):
        x = torch.randn(8, Fh, 1000, device=DEV).to(torch.bfloat16).requires_grad_(True)
        w = torch.randn(1, 1, K, Fh, device=DEV, requires_grad=True)
        ops.graph_filter_layer(x, w, None, graph, 'relu').sum().backward()
        assert x.grad is not None and w.grad is not None


def test_bf16_training_step_matches_fp32_composed_model():
    """One training step of a regression GCRNNGNN (F_h = 64, N = 1000, head [64, 1] K [5]) through fused_cell_train and the head
    kernel, against the same model in fp32 on the composed filter path, at the bf16 tolerances of tests/test_wide.py."""
    N, B, T = 1000, 2, 3
    S = sbm_uniform(N, 0)
    torch.manual_seed(7)
    m = archit.GatedGCRNNforRegression(64, 64, 5, 5, torch.tanh, torch.nn.ReLU, [], S[0], True, False, None, 'oneMlp',
                                       torch.nn.ReLU, [64, 1], [5], [N], gml.NoPool, [1]).float()
    ref = archit.GatedGCRNNforRegression(64, 64, 5, 5, torch.tanh, torch.nn.ReLU, [], S[0], True, False, None, 'oneMlp',
                                         torch.nn.ReLU, [64, 1], [5], [N], gml.NoPool, [1]).float()
    ref.load_state_dict(m.state_dict())
    m, ref = m.to(DEV), ref.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    X = torch.randn((B, T, 64, N), generator=gen, device=DEV).to(torch.bfloat16)
    h0 = torch.zeros((B, 64, N), device=DEV, dtype=torch.bfloat16)
    R = torch.randn((B, T, 1, N), generator=gen, device=DEV)
    assert m.stateGCRNN._use_fused_training(X, h0)
    (m(X, h0) * R).sum().backward()
    # reference: fp32 cell and the composed filter for the head
    with mock.patch.object(ops, 'graph_filter_layer_supported', lambda *a, **k: False):
        (ref(X.float(), h0.float()) * R).sum().backward()
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        a, r = p.grad.double().cpu().numpy(), q.grad.double().cpu().numpy()
        scale = max(1e-3, float(np.max(np.abs(r))))
        assert np.max(np.abs(a - r)) / scale <= 5e-2, (k, np.max(np.abs(a - r)), scale)


def test_g15_adam_trace_reproduced():
    g = load_golden('g15_trace_gcrnngnn')
    m = _model('g15_cls_gcrnngnn_none', g).double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params0'].items()})
    m = m.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    loss_fn = torch.nn.CrossEntropyLoss()
    h0 = torch.tensor(g['h0'], device=DEV)
    for it in range(10):
        m.zero_grad()
        loss = loss_fn(m(torch.tensor(g['x'][it], device=DEV), h0), torch.tensor(g['labels'][it], device=DEV))
        loss.backward()
        opt.step()
        assert abs(loss.item() - g['loss'][it]) <= 1e-9, (it, loss.item(), g['loss'][it])


def torch_filter_ref(x, w, b, S, act, dy):
    """fp64 forward and backward of one graph-filter layer with the dense S on the device (the numpy filter above, for sizes
    whose CPU evaluation would be slow): returns y, dx, dw, db."""
    dev = x.device
    Sd = torch.tensor(S, dtype=torch.float64, device=dev)
    xd = x.double().requires_grad_(True)
    wd = w.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True)
    z, pre = xd, 0
    for k in range(w.shape[2]):
        if k:
            z = z @ Sd
        pre = pre + torch.einsum('of,ifn->ion', wd[:, 0, k], z)
    y = {None: lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[act](pre + bd.reshape(1, -1, 1))
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), dy.double())
    return y.detach(), dx, dw, db


def _rel(a, ref):
    return float((a.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('Fin,Fout,K,act', [(20, 1, 4, 'relu'), (4, 8, 3, 'tanh')])
def test_many_items_per_workgroup_fp64_match_numpy(Fin, Fout, K, act):
    """Thousands of items on the N = 59 graph: every workgroup walks several items (grid-stride loop, barriers between items,
    dW / db accumulated over them); forward, dx, dW and db against the numpy fp64 filter. Both orders (taps first, hops first)."""
    S = np.load(os.path.join(GOLDEN, 'adj59.npy'))
    S = (S / np.max(np.abs(np.linalg.eigvals(S)))).reshape(1, 59, 59)
    graph = GraphOperator(S, device=DEV)
    items = 3000
    from gated_gcrnns_amd import _lib
    slots = _lib.lib.gcrnn_graph_filter_layer_wgrad_slots(_lib.F64, items, 59, graph.adj[0].nnz, Fin, Fout, K, 0)
    assert items >= 2 * slots, slots
    rng = np.random.default_rng(Fin + Fout)
    x = rng.standard_normal((items, Fin, 59))
    w = rng.uniform(-1, 1, (Fout, 1, K, Fin)) / np.sqrt(Fin * K)
    b = rng.uniform(-0.5, 0.5, (Fout, 1))
    dy = rng.standard_normal((items, Fout, 59))
    xd = torch.tensor(x, device=DEV, requires_grad=True)
    wd = torch.tensor(w, device=DEV, requires_grad=True)
    bd = torch.tensor(b, device=DEV, requires_grad=True)
    y = ops.graph_filter_layer(xd, wd, bd, graph, act)
    y.backward(torch.tensor(dy, device=DEV))
    yref, _ = np_filter(x, w, b, S[0], act)
    dx, dw, db = np_filter_backward(x, w, yref, dy, S[0], act)
    for a, r, what in ((y, yref, 'y'), (xd.grad, dx, 'dx'), (wd.grad, dw, 'dW'), (bd.grad, db, 'db')):
        err = _rel(a.detach().cpu(), torch.tensor(r))
        assert err <= 1e-11, (what, err)


@pytest.mark.parametrize('graph_kind', ['uniform', 'directed'])
def test_flagship_head_with_more_items_than_workgroups_bf16(graph_kind):
    """The flagship head (bf16 H, 64 -> 1, K = 5, N = 1000) with 1600 items: more than the 768 / 256 workgroup slots of the uniform
    / weighted graph, so each workgroup accumulates dW / db over several items. Against the fp64 filter of the same inputs."""
    N, Fin, Fout, K, items = 1000, 64, 1, 5, 1600
    S = sbm_uniform(N, 2) if graph_kind == 'uniform' else random_directed(N, 0.01, 7)
    graph = GraphOperator(S, device=DEV)
    from gated_gcrnns_amd import _lib
    uni = int(ops._gfl_uniform(graph.adj[0]) != 0.0)
    assert uni == (graph_kind == 'uniform')
    slots = _lib.lib.gcrnn_graph_filter_layer_wgrad_slots(_lib.BF16, items, N, graph.adj[0].nnz, Fin, Fout, K, uni)
    assert items > slots, slots
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((items, Fin, N), generator=gen, device=DEV).to(torch.bfloat16).requires_grad_(True)
    w = (torch.rand((Fout, 1, K, Fin), generator=gen, device=DEV) - 0.5).mul_(2 / (Fin * K) ** 0.5).requires_grad_(True)
    b = (0.1 * torch.randn((Fout, 1), generator=gen, device=DEV)).requires_grad_(True)
    dy = torch.randn((items, Fout, N), generator=gen, device=DEV)
    y = ops.graph_filter_layer(x, w, b, graph, 'relu')
    y.backward(dy)
    S32 = S[0].astype(np.float32).astype(np.float64)
    yref, dx, dw, db = torch_filter_ref(x.detach(), w, b, S32, 'relu', dy)
    assert _rel(y.detach(), yref) <= 1e-4
    assert _rel(x.grad, dx) <= 1e-2
    assert _rel(w.grad, dw) <= 2e-4, _rel(w.grad, dw)
    assert _rel(b.grad, db) <= 2e-4, _rel(b.grad, db)


@pytest.mark.parametrize('dtype,Fin,Fout,K', [(torch.float32, 64, 1, 5), (torch.float32, 4, 8, 3), (torch.bfloat16, 4, 8, 3),
                                              (torch.float32, 16, 4, 2)])
def test_vector_and_hops_first_paths_at_n1000(dtype, Fin, Fout, K):
    """fp32 at N = 1000 takes the 16-byte vector loads (N % 4 == 0); 4 -> 8 runs hops first, in fp32 and bf16; N = 998 (the last
    case) takes the scalar path of the same dtype. Forward, dx, dW, db against the fp64 filter, 900 items on the weighted graph."""
    N = 998 if Fin == 16 else 1000
    S = random_directed(N, 0.008, 11)
    graph = GraphOperator(S, device=DEV)
    items = 900
    gen = torch.Generator(device=DEV).manual_seed(Fin * 7 + K)
    x = torch.randn((items, Fin, N), generator=gen, device=DEV).to(dtype).requires_grad_(True)
    w = (torch.rand((Fout, 1, K, Fin), generator=gen, device=DEV) - 0.5).mul_(2 / (Fin * K) ** 0.5).requires_grad_(True)
    b = (0.1 * torch.randn((Fout, 1), generator=gen, device=DEV)).requires_grad_(True)
    dy = torch.randn((items, Fout, N), generator=gen, device=DEV)
    assert ops.graph_filter_layer_supported(dtype, torch.float32, graph, Fin, Fout, K)
    y = ops.graph_filter_layer(x, w, b, graph, 'sigmoid')
    y.backward(dy)
    S32 = S[0].astype(np.float32).astype(np.float64)
    yref, dx, dw, db = torch_filter_ref(x.detach(), w, b, S32, 'sigmoid', dy)
    assert _rel(y.detach(), yref) <= 1e-5
    assert _rel(x.grad, dx) <= (1e-2 if dtype == torch.bfloat16 else 1e-5)
    assert _rel(w.grad, dw) <= 2e-4 and _rel(b.grad, db) <= 2e-4, (_rel(w.grad, dw), _rel(b.grad, db))


def test_sel_and_gcrnngnn_train_through_the_harness(tmp_path):
    """MultipleModels trains a 'Sel' model (the reference's non-recurrent branch: x viewed as (B*T) x 1 x N, archit(x)) next to a
    'GCRNNGNN' model on the same batches; both take optimiser steps and keep finite losses."""
    from gated_gcrnns_amd.Modules.train_rnn import MultipleModels, TrainableModel
    from gated_gcrnns_amd.Utils import miscTools
    N, T, nTrain = 20, 4, 8
    S = random_directed(N, 0.3, 2)[0]
    torch.manual_seed(0)
    # (tanh layers, no final ReLU: a ReLU output layer that is dead on every node of a tiny random problem would leave the parameters
    # where they were and prove nothing about the harness)
    sel = archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.Tanh, [N, N], gml.NoPool, [1, 1], [], S).to(DEV)
    gnn = archit.GatedGCRNNforRegression(1, 8, 3, 3, torch.tanh, torch.nn.Tanh, [], S, True, False, None, 'oneMlp', None,
                                         [8, 1], [3], [N], gml.NoPool, [1]).to(DEV)
    models = {name: TrainableModel(m, miscTools.batchTimeL1Loss, torch.optim.Adam(m.parameters(), lr=1e-2), name, str(tmp_path))
              for name, m in (('Sel', sel), ('GCRNNGNN', gnn))}
    before = {k: [p.detach().clone() for p in tm.archit.parameters()] for k, tm in models.items()}
    rng = np.random.default_rng(0)
    xT = torch.tensor(rng.standard_normal((nTrain, T, N)), dtype=torch.float32)
    yT = torch.tensor(rng.standard_normal((nTrain, T, N)), dtype=torch.float32)
    out = MultipleModels(models, xT, yT, xT, yT, 1, 4, T, 8, miscTools.batchTimeMSELoss, validationInterval=1,
                         rng=np.random.RandomState(0))
    for k, tm in models.items():
        assert len(out['lossTrain'][k]) == 2 and np.isfinite(out['lossTrain'][k]).all() and np.isfinite(out['evalValid'][k]).all()
        assert any(not torch.equal(p, q) for p, q in zip(tm.archit.parameters(), before[k])), k


def test_examples_accept_the_gnn_models():
    import importlib.util
    from conftest import ROOT
    prev = torch.get_default_dtype()
    try:
        spec = importlib.util.spec_from_file_location('kstep_example_gnn', os.path.join(ROOT, 'examples', 'kstep_prediction.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        res = mod.main(['--nodes', '30', '--seq', '3', '--ntrain', '200', '--batch', '50', '--models', 'Sel,GCRNNGNN,TimeGCRNNGNN'])
        assert sorted(res) == ['GCRNNGNN', 'Sel', 'TimeGCRNNGNN'] and all(np.isfinite(r['score']) for r in res.values())
        spec = importlib.util.spec_from_file_location('epicenter_example_gnn', os.path.join(ROOT, 'examples', 'epicenter_estimation.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        res = mod.main(['--steps', '5', '--seq', '20', '--taps', '4', '--models', 'Sel,GCRNNGNN'])
        assert sorted(res) == ['GCRNNGNN', 'Sel'] and all(np.isfinite(r['loss']).all() for r in res.values())
    finally:
        torch.set_default_dtype(prev)
