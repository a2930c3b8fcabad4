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


# ---------------------------------------------------------------------------------------------- G19: the edge gate's softmax at its extremes
ATT_REGIMES = ['zero', 'default', 'peaked', 'mixed']
CELL_SETTINGS = ['zero_zero', 'peaked_peaked', 'zero_peaked', 'default_default']
VANISHED = 1e-3      # a reference gradient below this share of the SAME gradient's max under the default initialisation counts as vanished (a
                     # saturated softmax scales it by alpha (1 - alpha)); it is then held absolutely, to the bound times that default-init max


def regime_grad_err(g, ref, ref_default):
    """Max-abs error of one gradient over the magnitude it is held to: its reference's own max, or -- where that has vanished -- the max of the
    same gradient in the default-init regime (never the vanished gradient's own rounding noise)."""
    ref, dflt = np.asarray(ref, dtype=np.float64), float(np.max(np.abs(ref_default)))
    own = float(np.max(np.abs(ref)))
    scale = own if own >= VANISHED * dflt else dflt
    g = g.detach().cpu().double().numpy() if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64)
    assert np.all(np.isfinite(g))
    return float(np.max(np.abs(g - ref))) / (scale + 1e-300)


def test_g19_fixture_is_on_the_dir17_graph_and_holds_the_regimes_it_names():
    """The stored graph is tests/test_small_edge_train.py::gso_dir17 bit for bit; the zero regime's scores are exactly 0 with Wx != 0, the
    mixed regime's are exactly 0 on part of the support and of both signs on the rest (exact dyadic operands), and the peaked regimes have
    at least 30 % of their support rows of two or more entries one-hot to 1e-6."""
    from test_small_edge_train import gso_dir17
    g = load_golden('g19_attention_regimes')
    S = g['S']
    assert np.array_equal(S, gso_dir17())
    N = S.shape[1]
    mask = np.abs(S[0] + np.eye(N)) > tr.ZERO_TOLERANCE
    assert mask[3].sum() == 0 and mask[5].sum() == 1 and mask[:, 5].sum() == 1 and mask[9].sum() == N - 1      # empty row, isolated node, hub row

    def scores(r):
        F = r['W'].shape[2]
        Wx = np.einsum('fg,bgn->bfn', r['W'][0, 0], r['x'])
        s1, s2 = np.einsum('f,bfn->bn', r['a'][0, 0, :F], Wx), np.einsum('f,bfn->bn', r['a'][0, 0, F:], Wx)
        return (s1[:, None, :] + s2[:, :, None])[:, mask], Wx
    z, Wx = scores(g['att_zero'])
    assert np.all(z == 0) and np.abs(Wx).min() > 0
    z, _ = scores(g['att_mixed'])
    assert (z == 0).sum() > 2 * mask.diagonal().sum() and (z > 0).sum() >= 10 and (z < 0).sum() >= 10
    assert np.array_equal(z * 256, np.round(z * 256))
    r = g['att_peaked']
    assert np.array_equal(r['a'], float(g['att_k']) * g['att_default']['a']) and float(g['att_k']) > 1
    y = tr.graph_attention(t64(r['x']), t64(r['a']), t64(r['W']), t64(S))            # (finite at scores of this size)
    assert bool(torch.isfinite(y).all())
    for s in CELL_SETTINGS:
        p = g['cell_%s_params' % s]
        for att, kind in zip(('input_attention', 'forget_attention'), s.split('_')):
            want = {'zero': 0.0, 'peaked': float(g['cell_k']), 'default': 1.0}[kind] * g['cell_default_default_params'][att + '.mixer']
            assert np.array_equal(p[att + '.mixer'], want), (s, att)
    b = g['cell_peaked_peaked_params']['bias'][:, 0]
    for i, att in enumerate(('input_attention', 'forget_attention')):
        a, W = g['cell_peaked_peaked_params'][att + '.mixer'][0, 0], g['cell_peaked_peaked_params'][att + '.weight'][0, 0]
        assert abs((a[:7] + a[7:]) @ (W @ b) - g['cell_peaked_offset'][i]) <= 1e-12 * abs(g['cell_peaked_offset'][i])


@pytest.mark.parametrize('regime', ATT_REGIMES)
def test_g19_graph_attention_values_and_gradients(regime):
    """tr.graph_attention against the reference's graphAttention in every regime: values to 1e-12, the gradients w.r.t. x, a and W to 1e-10
    of each gradient's max. a = 0 is the LeakyReLU's kink: a derivative of 1 there gives a mixer gradient five times the reference's."""
    g = load_golden('g19_attention_regimes')
    r, d = g['att_' + regime], g['att_default']
    x, a, W = t64(r['x'], True), t64(r['a'], True), t64(r['W'], True)
    y = tr.graph_attention(x, a, W, t64(g['S']))
    assert tuple(y.shape) == r['y'].shape and maxdiff(y, r['y']) <= TOL
    (y * t64(g['att_R'])).sum().backward()
    for name, got in (('grad_x', x.grad), ('grad_a', a.grad), ('grad_W', W.grad)):
        e = regime_grad_err(got, r[name], d[name])
        assert e <= GTOL, (regime, name, e)
    if regime == 'zero':
        assert float(np.abs(r['grad_a']).max()) > 0.1                               # (the kink's gradient is not a zero that hides the factor)


@pytest.mark.parametrize('setting', CELL_SETTINGS)
def test_g19_edge_gated_cell_states_and_gradients(setting):
    """tr.ggcrnn_cell(spatial_gating='edge') against the reference cell with zero / peaked / default mixers: states to 1e-12, every
    parameter's, h0's and X's gradient to 1e-10 of its max (a vanished one: of its max under the default initialisation)."""
    g = load_golden('g19_attention_regimes')
    p = params64(g['cell_%s_params' % setting], True)
    X, h0 = t64(g['cell_X'], True), t64(g['cell_h0'], True)
    H = tr.ggcrnn_cell(p, t64(g['S']), X, h0, False, 'edge')
    assert maxdiff(H, g['cell_%s_H' % setting]) <= TOL
    (H * t64(g['cell_R'])).sum().backward()
    ref, dflt = g['cell_%s_grads' % setting], g['cell_default_default_grads']
    got = {k: v.grad for k, v in p.items()}
    got.update(h0=h0.grad, X=X.grad)
    assert set(ref) == set(got) and len(ref) == 9
    for k in sorted(ref):
        e = regime_grad_err(got[k], ref[k], dflt[k])
        assert e <= GTOL, (setting, k, e)
