"""CPU: the plain-torch fp64 reference (oracle/torch_reference.py) against the numpy oracle and the reference's own fixtures.

Forward: equal to oracle/gcrnn_oracle.py to 1e-12 on every fixture the oracle is pinned to, and to the reference's stored states where the
oracle is not checked (G13, G14). Gradients: torch autograd through the dense restatement equals the reference's autograd gradients stored
in the fixtures to 1e-10 of each gradient's max. This ties the torch reference to the reference without a GPU; tests/test_fp64_envelopes.py
then ties every fp64 kernel path of this library to the torch reference."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import gcrnn_oracle as orc
from oracle import torch_reference as tr

TOL = 1e-12
GTOL = 1e-10
VARIANTS = [('none', False, None), ('time', True, None), ('node', False, 'node'),
            ('edge', False, 'edge'), ('time_node', True, 'node'), ('time_edge', True, 'edge')]


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def params64(p, grad=False):
    return {k: t64(v, grad) for k, v in p.items()}


def maxdiff(a, ref):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.max(np.abs(a - np.asarray(ref, dtype=np.float64))))


def relgrad(g, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(g.detach().numpy() - ref)) / (np.max(np.abs(ref)) + 1e-30))


def coo_gso(g):
    N = int(g['shape'][0])
    S = np.zeros((1, N, N))
    S[0, g['coo_row'].astype(np.int64), g['coo_col'].astype(np.int64)] = g['coo_val'].astype(np.float64)
    return S


def check_grads(params, ref, tol=GTOL):
    """Every parameter the fixture holds a gradient for; parameters the forward does not use (GFL_out / MLP_out) get none."""
    assert ref
    for k, v in ref.items():
        assert params[k].grad is not None, k
        assert relgrad(params[k].grad, v) <= tol, (k, relgrad(params[k].grad, v))
    for k, p in params.items():
        if k.startswith(('GFL_out.', 'MLP_out.')):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


def test_g1_lsigf_forward_and_gradients():
    g = load_golden('g1_lsigf')
    h, x, b = t64(g['h'], True), t64(g['x'], True), t64(g['b'], True)
    S = t64(g['S'])
    y = tr.lsigf(h, S, x, b)
    assert maxdiff(y, orc.lsigf(g['h'], g['S'], g['x'], g['b'])) <= TOL
    assert maxdiff(y, g['y_bias']) <= TOL
    assert maxdiff(tr.lsigf(h, S, x), g['y_nobias']) <= TOL
    y2 = tr.lsigf(t64(g['h2']), t64(g['S2']), x, b)                 # E = 2 edge features
    assert maxdiff(y2, orc.lsigf(g['h2'], g['S2'], g['x'], g['b'])) <= TOL and maxdiff(y2, g['y_e2']) <= TOL
    (y * t64(g['r'])).sum().backward()
    assert relgrad(h.grad, g['grad_h']) <= GTOL
    assert relgrad(x.grad, g['grad_x']) <= GTOL
    assert relgrad(b.grad, g['grad_b']) <= GTOL


def test_g2_graph_filter_zero_pad():
    g = load_golden('g2_graphfilter')
    p = g['params']
    w, b, S = t64(p['weight']), t64(p['bias']), t64(g['S'])
    assert maxdiff(tr.graph_filter(w, b, S, t64(g['x'])), g['y']) <= TOL
    ys = tr.graph_filter(w, b, S, t64(g['x_short']))
    assert tuple(ys.shape) == g['y_short'].shape
    assert maxdiff(ys, g['y_short']) <= TOL
    assert maxdiff(ys, orc.graph_filter(p['weight'], p['bias'], g['S'], g['x_short'])) <= TOL


@pytest.mark.parametrize('act', [None, 'relu', 'tanh', 'sigmoid'])
def test_graph_filter_layer_is_the_activated_filter(act):
    """graph_filter_layer = act(LSIGF) on a directed weighted graph: the oracle's filter with the numpy activation."""
    rng = np.random.default_rng(3)
    N, Fin, Fout, K, items = 23, 4, 3, 3, 5
    S = (rng.random((1, N, N)) < 0.2) * rng.standard_normal((1, N, N))
    w, b, x = rng.standard_normal((Fout, 1, K, Fin)), rng.standard_normal((Fout, 1)), rng.standard_normal((items, Fin, N))
    y = tr.graph_filter_layer(t64(w), t64(b), t64(S), t64(x), act)
    pre = orc.lsigf(w, S, x, b)
    want = {None: pre, 'relu': np.maximum(pre, 0.0), 'tanh': np.tanh(pre), 'sigmoid': orc.sigmoid(pre)}[act]
    assert maxdiff(y, want) <= TOL


def test_graph_attentional_matches_oracle():
    rng = np.random.default_rng(4)
    N, G, F, K, B = 19, 3, 4, 2, 2
    S = (rng.random((1, N, N)) < 0.25) * rng.standard_normal((1, N, N))
    S[0, 2, :] = 0.0
    S[0, :, 2] = 0.0                                                # isolated node: only its self-loop is in the support
    S[0, 5, 5] = -1.0                                               # (S + I)[5][5] = 0 leaves the support
    mixer, weight, x = rng.standard_normal((K, 1, 2 * F)), rng.standard_normal((K, 1, F, G)), rng.standard_normal((B, G, N))
    y = tr.graph_attentional(t64(mixer), t64(weight), t64(S), t64(x))
    assert maxdiff(y, orc.graph_attentional(mixer, weight, S, x)) <= TOL


@pytest.mark.parametrize('name,tg,sg', VARIANTS)
def test_g3_g4_cell_states_and_gradients(name, tg, sg):
    g = load_golden('g3_cell_' + name)
    p = params64(g['params'], True)
    X, h0 = t64(g['X'], True), t64(g['h0'], True)
    S = t64(g['S'])
    H = tr.ggcrnn_cell(p, S, X, h0, tg, sg)
    assert maxdiff(H, orc.ggcrnn_cell(g['params'], g['S'], g['X'], g['h0'], tg, sg)) <= TOL
    assert maxdiff(H, g['H']) <= TOL
    H.sum().backward(retain_graph=True)
    check_grads(p, g['grad_sum'])
    assert relgrad(X.grad, g['grad_sum_X']) <= GTOL
    assert relgrad(h0.grad, g['grad_sum_h0']) <= GTOL
    for q in list(p.values()) + [X, h0]:
        q.grad = None
    torch.nn.L1Loss()(H, t64(g['target'])).backward()
    check_grads(p, g['grad_l1'])
    assert relgrad(X.grad, g['grad_l1_X']) <= GTOL


@pytest.mark.parametrize('name,tg', [('none', False), ('time', True)])
def test_g3_cell_no_bias_unequal_taps(name, tg):
    g = load_golden('g3_cell_%s_nobias' % name)
    H = tr.ggcrnn_cell(params64(g['params']), t64(g['S']), t64(g['X']), t64(g['h0']), tg, None)
    assert maxdiff(H, orc.ggcrnn_cell(g['params'], g['S'], g['X'], g['h0'], tg, None)) <= TOL
    assert maxdiff(H, g['H']) <= TOL


@pytest.mark.parametrize('fixture,tg', [('g5_reg_oneMlp_none', False), ('g5_reg_oneMlp_time', True), ('g5_reg_multipMlp_none', False),
                                        ('g5_reg_multipMlp_time', True), ('g5_cls_T20K4_none', False), ('g5_cls_T20K4_time', True),
                                        ('g5_cls_T200K3_none', False), ('g5_cls_T200K3_time', True)])
def test_g5_cell_states_equal_oracle(fixture, tg):
    """G5 (the drivers' shapes, incl. the directed 59-node seismic graph at T = 200): the state cell of each model equals the oracle's."""
    g = load_golden(fixture)
    cell = {k[len('stateGCRNN.'):]: v for k, v in g['params'].items() if k.startswith('stateGCRNN.')}
    H = tr.ggcrnn_cell(params64(cell), t64(g['S']), t64(g['x']), t64(g['h0']), tg, None)
    assert maxdiff(H, orc.ggcrnn_cell(cell, g['S'], g['x'], g['h0'], tg, None)) <= TOL


def test_g8_midsize_states_equal_oracle():
    g = load_golden('g8_mid')
    N, B, Tn, G, F, K = [int(v) for v in g['shape']]
    S = np.zeros((1, N, N))
    S[0, g['coo_row'], g['coo_col']] = g['coo_val']
    X = np.random.default_rng(int(g['x_seed'][0])).standard_normal((B, Tn, G, N))
    H = tr.ggcrnn_cell(params64(g['params']), t64(S), t64(X), torch.zeros(B, F, N, dtype=torch.float64)).numpy()
    assert np.max(np.abs(H.reshape(-1)[g['sample_idx']] - g['sample_val'])) <= 1e-11
    assert np.max(np.abs(H[0, 3, 0] - g['H_b0_t3_f0'])) <= 1e-11
    assert maxdiff(H, orc.ggcrnn_cell(g['params'], S, X, np.zeros((B, F, N)))) <= TOL


@pytest.mark.parametrize('name,tg,sg', VARIANTS[:4] + VARIANTS[5:])
def test_g9_states_and_gradients(name, tg, sg):
    """G9: bf16-representable operands, directed weighted graph. The fixture stores states and gradients rounded to fp32, so they are
    compared at fp32 rounding (2e-7 of their max); the oracle, on the same operands, at 1e-12."""
    g = load_golden('g9_fused_' + name)
    S = coo_gso(g)
    p = {k: v.astype(np.float64) for k, v in g['params'].items()}
    pt = params64(p, True)
    X, h0 = t64(g['X'], True), t64(g['h0'], True)
    H = tr.ggcrnn_cell(pt, t64(S), X, h0, tg, sg)
    assert maxdiff(H, orc.ggcrnn_cell(p, S, g['X'].astype(np.float64), g['h0'].astype(np.float64), tg, sg)) <= TOL
    assert maxdiff(H, g['H']) <= 2e-7
    H.sum().backward()
    check_grads(pt, g['grad_sum'], tol=2e-7)
    assert relgrad(h0.grad, g['grad_sum_h0']) <= 2e-7
    assert relgrad(X.grad, g['grad_sum_X']) <= 2e-7


@pytest.mark.parametrize('fixture,tg,sg', [('g11_fused_f32', False, None), ('g12_fused_f32_time', True, None),
                                           ('g13_fused_f32_node', False, 'node'), ('g13_fused_f32_time_node', True, 'node'),
                                           ('g14_fused_f32_edge', False, 'edge'), ('g14_fused_f32_time_edge', True, 'edge')])
def test_g11_to_g14_states_and_gradients(fixture, tg, sg):
    """G11-G14 (fp32-representable operands, fp64 reference states and autograd gradients): states to 1e-12 of the reference's (G13 and G14
    are the node- and edge-gated states the oracle tests do not check), every stored gradient to 1e-10 of its max."""
    g = load_golden(fixture)
    S = coo_gso(g)
    pt = params64(g['params'], True)
    X, h0 = t64(g['X']), t64(g['h0'], True)
    H = tr.ggcrnn_cell(pt, t64(S), X, h0, tg, sg)
    assert maxdiff(H, g['H']) <= TOL
    if fixture.startswith(('g11', 'g12')):
        assert maxdiff(H, orc.ggcrnn_cell({k: v.astype(np.float64) for k, v in g['params'].items()}, S, g['X'].astype(np.float64),
                                          g['h0'].astype(np.float64), tg, sg)) <= TOL
    if 'grad_sum' not in g:
        return
    H.sum().backward(retain_graph=True)
    check_grads(pt, g['grad_sum'])
    if 'grad_sum_h0' in g:
        assert relgrad(h0.grad, g['grad_sum_h0']) <= GTOL
    if 'grad_l1' in g:
        for q in list(pt.values()) + [h0]:
            q.grad = None
        torch.nn.L1Loss()(H, t64(g['target'])).backward()
        check_grads(pt, g['grad_l1'])
        if 'grad_l1_h0' in g:
            assert relgrad(h0.grad, g['grad_l1_h0']) <= GTOL


def _g15_forward(name, p, S, ins):
    """The G15 models (tests/test_gnn_heads.py builds the same ones): a Selection-GNN head with ReLU layers, after the state cell."""
    if name.startswith('g15_sel'):
        return tr.selection_gnn(p, S, ins[0])
    cell = tr._sub(p, 'stateGCRNN.')
    head = tr._sub(p, 'outputNN.0.')
    H = tr.ggcrnn_cell(cell, S, ins[0], ins[1], name.endswith('time'), None)
    B, T, F, N = H.shape
    if name.startswith('g15_cls'):
        return torch.relu(tr.selection_gnn(head, S, H[:, -1]))
    return torch.relu(tr.selection_gnn(head, S, H.reshape(B * T, F, N))).reshape(B, T, -1).unsqueeze(2)


@pytest.mark.parametrize('name', ['g15_sel_quake', 'g15_sel_kstep', 'g15_cls_gcrnngnn_none', 'g15_cls_gcrnngnn_time',
                                  'g15_reg_gcrnngnn_none', 'g15_reg_gcrnngnn_time', 'g15_reg_gcrnngnn_deep'])
def test_g15_models_outputs_and_gradients(name):
    g = load_golden(name)
    pt = params64(g['params'], True)
    S = t64(g['S'])
    ins = [t64(g['x'], True)] + ([t64(g['h0'], True)] if 'h0' in g else [])
    y = _g15_forward(name, pt, S, ins)
    assert tuple(y.shape) == g['y'].shape
    assert maxdiff(y, g['y']) <= TOL * max(1.0, float(np.abs(g['y']).max()))
    (y * t64(g['R'])).sum().backward()
    check_grads(pt, g['grads'])
    assert relgrad(ins[0].grad, g['grad_x']) <= GTOL
    if len(ins) > 1:
        assert relgrad(ins[1].grad, g['grad_h0']) <= GTOL


def test_the_reference_keeps_its_inputs_dtype():
    g = load_golden('g3_cell_time')
    p = {k: torch.tensor(v, dtype=torch.float32) for k, v in g['params'].items()}
    H = tr.ggcrnn_cell(p, torch.tensor(g['S'], dtype=torch.float32), torch.tensor(g['X'], dtype=torch.float32),
                       torch.tensor(g['h0'], dtype=torch.float32), True, None)
    assert H.dtype == torch.float32 and H.device.type == 'cpu'
    assert maxdiff(H.double(), g['H']) <= 1e-5
