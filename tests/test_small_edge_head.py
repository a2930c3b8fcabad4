"""GPU (-m gpu): the edge-gated models on small graphs with their output head inside the recurrence launches --
gcrnn_small_edge_forward_head (read-out on the last state / per-node head on every state, state-store modes),
gcrnn_small_edge_backward_head (BPTT whose upstream comes from dlogits / dY), ops.small_edge_cell_classify / _regress,
GGCRNNCell.classify / regress under GCRNN_SMALL_EDGE_HEAD=1 and the two models' forward.

What is compared with what:
  states    the new entry's stores against ops.small_edge_cell_forward (same arithmetic: torch.equal); no store: no H, the same output bits.
  logits    against torch.nn.functional.linear in fp64 on the existing path's h_T: two summation orders of F N terms differ by at most
            2 F N eps sum|w h| per element; the test computes it.
  y         against ops.node_linear on the existing path's states: 2 F eps sum_f |w h| per element.
  backward  dlogits / dY are multiples of 1/4 in [-2, 2], head_w / node_w multiples of 1/8 in [-1, 1], none zero: every partial sum is a
            multiple of 1/32 far below 2^10, exact in both dtypes in any order, so the new backward must equal the existing one fed
            the equivalent dH bit for bit.
  model     oracle.gated_gcrnn_classification / _regression (1e-11 fp64, 1e-5 fp32) and oracle/torch_reference.ggcrnn_cell plus a torch head
            under CPU fp64 autograd (states and outputs 1e-11 / 1e-5, each gradient 1e-10 / 2e-5 of its maximum).
Every case uses a non-zero h0 and seeded inputs (GraphedTrainStep alone starts from its own zero state)."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from oracle import torch_reference as tr
from test_small_head import _CountingLib, _adj59, _gso, _spread
from test_small_edge import gso_dir17, gso_sbm50

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64, F32 = torch.float64, torch.float32
FWD_HEAD, BWD_HEAD = 'gcrnn_small_edge_forward_head', 'gcrnn_small_edge_backward_head'
E_FWD, E_BWD, E_DX = 'gcrnn_small_edge_forward', 'gcrnn_small_edge_backward', 'gcrnn_small_edge_backward_dx'
NL_FWD, NL_BWD = 'gcrnn_node_linear_forward', 'gcrnn_node_linear_backward'
SWITCH = 'GCRNN_SMALL_EDGE_HEAD'
TOL = {F64: 1e-11, F32: 1e-5}                              # test_small_edge.py::TOL
TOLS = {F64: (1e-11, 1e-10), F32: (1e-5, 2e-5)}            # test_small_edge_train.py::TOLS: states / outputs, gradients (of their maximum)



def _switch_on(monkeypatch, kind, dt):
    """GCRNN_SMALL_EDGE_HEAD=1; for the fp64 per-node head, which the timing rule takes off that dispatch (GGCRNNCell._small_edge_head_pays),
    =all: its path is tested all the same."""
    monkeypatch.setenv(SWITCH, 'all' if kind == 'reg' and dt == F64 else '1')


ENV = (SWITCH, 'GCRNN_NO_SMALL_EDGE', 'GCRNN_NO_SMALL_HEAD', 'GCRNN_NO_SMALL_NODE_HEAD', 'GCRNN_SMALL_EDGE_DX', 'GCRNN_SMALL_GATHER')


def ops():
    from gated_gcrnns_amd import ops as m
    return m


def archit():
    import gated_gcrnns_amd.Modules.architectures as m
    return m


@pytest.fixture
def spy(monkeypatch):
    """Counts the library's entry points and the Python wrappers the recurrence and the head can go through."""
    o = ops()
    s = _CountingLib(o.lib)
    monkeypatch.setattr(o, 'lib', s)
    for name in ('small_edge_cell_forward', 'small_edge_cell_train', 'small_edge_cell_classify', 'small_edge_cell_regress', 'node_linear'):
        def wrap(fn, name):
            def counted(*a, **kw):
                s.calls[name] += 1
                return fn(*a, **kw)
            return counted
        monkeypatch.setattr(o, name, wrap(getattr(o, name), name))
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    return s


# ------------------------------------------------------------------------------------------------------------------ kernel level
#          N,   G, F,  Kin, Kst, T, B, O, C
SHAPES = {'quake59': (59, 1, 20, 4, 4, 3, 3, 1, 11),       # F N = 1180 > 1024: two thread passes
          'tiny': (16, 9, 4, 2, 4, 2, 2, 3, 17),           # G > F, Kin < Kst, one pass; more classes than the 16 waves
          't1': (17, 1, 5, 3, 2, 1, 1, 2, 3),              # T = 1: the only y is the one behind the loop; the backward has one step
          'five80': (80, 1, 20, 5, 5, 4, 2, 1, 11),        # the k-step driver's graph size
          'full128': (128, 1, 30, 2, 2, 2, 2, 8, 11),      # fp32 only: (F + 2) N = 4096 and O N = 1024, both exactly at the kernel's limits
          'signed': (17, 3, 7, 1, 1, 3, 2, 2, 5)}          # the directed signed graph: empty support row, isolated node, hub; K = 1, no bias
SALT = {'tiny': 1}                                          # a seed at which the read-out's gradient reaches h0 through both steps' ReLUs
CASES = [(s, dt) for s in ('quake59', 'tiny', 't1', 'five80', 'signed') for dt in (F64, F32)] + [('full128', F32)]


def kernel_cases(fn):
    """Every shape and dtype, with and without bias (the cell's and the head's), with no gates and [T][B] time gates."""
    fn = pytest.mark.parametrize('shape,dt', CASES, ids=['%s-%s' % (s, 'f64' if dt == F64 else 'f32') for s, dt in CASES])(fn)
    fn = pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])(fn)
    return pytest.mark.parametrize('gates', ['none', 'time'])(fn)


def _ring80():
    """N = 80, directed and signed, two entries per row (a ring and one seeded edge): the fp64 BPTT image of K = 5 fits its 150 KiB."""
    rng = np.random.default_rng(80)
    N = 80
    M = np.zeros((N, N))
    for n in range(N):
        M[n, (n + 1) % N] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0])
        M[n, (n + 7 + int(rng.integers(0, 50))) % N] = rng.uniform(0.3, 1.0)
    return M / np.abs(M).sum(axis=1).max()


def _graph_of(shape, N):
    if shape == 'signed':
        return gso_dir17()
    return (_ring80() if shape == 'five80' else _gso(N))[None]


@functools.lru_cache(maxsize=None)
def _case(shape, dt, bias, gates):
    """Seeded operands of one kernel-level case on the device and (computed once, never written again) the existing kernel's states."""
    from gated_gcrnns_amd.graph import GraphOperator
    o = ops()
    N, G, F, Kin, Kst, T, B, O, C = SHAPES[shape]
    gen = torch.Generator().manual_seed(13 * N + 5 * T + B + SALT.get(shape, 0))

    def r(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    def u(*s):
        return torch.rand(*s, generator=gen, dtype=F64)

    def q(lo, hi, step, *s):                               # multiples of 1 / step in [lo, hi], none of them zero
        v = torch.randint(int(lo * step), int(hi * step) + 1, s, generator=gen).double()
        return torch.where(v == 0, torch.ones_like(v), v) / step
    c = dict(N=N, G=G, F=F, Kin=Kin, Kst=Kst, T=T, B=B, O=O, C=C, dt=dt)
    c['graph'] = GraphOperator(_graph_of(shape, N), device=DEV)
    t = dict(X=r(B, T, G, N), h0=0.5 * r(B, F, N), wA=(2 * u(F, 1, Kin, G) - 1) / np.sqrt(G * Kin), wB=(2 * u(F, 1, Kst, F) - 1) / np.sqrt(F * Kst),
             b=0.2 * r(F, 1), m_in=r(1, 1, 2 * F) / np.sqrt(F), w_in=r(1, 1, F, F) / np.sqrt(F), m_f=r(1, 1, 2 * F) / np.sqrt(F),
             w_f=r(1, 1, F, F) / np.sqrt(F), gi=0.1 + 0.8 * u(T, B), gf=0.1 + 0.8 * u(T, B),
             head_w=q(-1, 1, 8, C, F * N), head_b=r(C), dlogits=q(-2, 2, 4, B, C),
             node_w=q(-1, 1, 8, O, F), node_b=(1.0 + u(O)) * torch.where(u(O) < 0.5, -1.0, 1.0), dY=q(-2, 2, 4, B, T, O, N))
    for k, v in t.items():
        c[k] = v.to(DEV).to(dt)
    if not bias:
        c['b'] = c['head_b'] = c['node_b'] = None
    if shape == 'signed':
        c['b'] = None
    if gates == 'none':
        c['gi'] = c['gf'] = None
    assert float(c['h0'].abs().min()) > 0
    nnz, nnzs = c['graph'].fwd[0].nnz, c['graph'].edge_plan()['nnz']
    # never skipped on a no: the shapes were chosen inside the kernels' envelope
    for kind, NC in ((o.SMALL_EDGE_HEAD_LAST, C), (o.SMALL_EDGE_HEAD_NODE, O)):
        assert o.small_edge_head_supported(N, nnz, nnzs, G, F, Kin, Kst, kind, NC, dt, False), shape
        assert o.small_edge_head_supported(N, nnz, nnzs, G, F, Kin, Kst, kind, NC, dt, True), shape
    with torch.no_grad():
        c['H'] = o.small_edge_cell_forward(*_cell_args(c), c['gi'], c['gf'])
        c['H_last'] = o.small_edge_cell_forward(*_cell_args(c), c['gi'], c['gf'], last_only=True)
    assert torch.equal(c['H'][:, -1:], c['H_last'])
    return c


def _cell_args(c, leaf=None):
    s = c if leaf is None else leaf
    return (s['X'], s['h0'], s['wA'], s['wB'], s['b'], c['graph'], (s['m_in'], s['w_in']), (s['m_f'], s['w_f']))


def _head_forward(c, kind, store, head_bias=True):
    o = ops()
    w, b = (c['head_w'], c['head_b']) if kind == o.SMALL_EDGE_HEAD_LAST else (c['node_w'], c['node_b'])
    X, h0, wA, wB, bb, graph, att_in, att_f = _cell_args(c)
    return o._small_edge_forward_head(X, h0, wA, wB, bb, graph, att_in, att_f, c['gi'], c['gf'], kind, w, b if head_bias else None, store)


@kernel_cases
def test_state_stores_keep_the_existing_bits(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    assert _spread(c['H']) and bool(torch.isfinite(c['H']).all())
    for kind, oshape in ((o.SMALL_EDGE_HEAD_LAST, (c['B'], c['C'])), (o.SMALL_EDGE_HEAD_NODE, (c['B'], c['T'], c['O'], c['N']))):
        H_all, y_all = _head_forward(c, kind, o.SMALL_STATES_ALL)
        H_last, y_last = _head_forward(c, kind, o.SMALL_STATES_LAST)
        H_none, y_none = _head_forward(c, kind, o.SMALL_STATES_NONE)
        assert tuple(H_all.shape) == (c['B'], c['T'], c['F'], c['N']) and torch.equal(H_all, c['H'])
        assert tuple(H_last.shape) == (c['B'], 1, c['F'], c['N']) and torch.equal(H_last, c['H_last'])
        assert H_none is None
        assert tuple(y_all.shape) == oshape and bool(torch.isfinite(y_all).all()) and _spread(y_all)
        assert torch.equal(y_all, y_none) and torch.equal(y_all, y_last)              # the output does not depend on what is stored
        assert torch.equal(y_none, _head_forward(c, kind, o.SMALL_STATES_NONE)[1])    # fixed order: two runs, the same bits


@kernel_cases
def test_logits_within_the_summation_order_bound(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    B, FN = c['B'], c['F'] * c['N']
    logits = _head_forward(c, o.SMALL_EDGE_HEAD_LAST, o.SMALL_STATES_NONE)[1]
    h = c['H_last'].reshape(B, FN).double()
    ref = torch.nn.functional.linear(h, c['head_w'].double(), c['head_b'].double() if c['head_b'] is not None else None)
    bound = 2.0 * FN * torch.finfo(dt).eps * (h.abs() @ c['head_w'].double().abs().t())
    if c['head_b'] is not None:                            # the rounding of the final addition of the bias
        bound = bound + torch.finfo(dt).eps * ref.abs()
    err = (logits.double() - ref).abs()
    print('%s %s: max|logits - linear| = %.3g, max err / bound = %.3g' % (shape, dt, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    if bias:                                               # the bias is there: without it every logit moves by head_b
        bare = _head_forward(c, o.SMALL_EDGE_HEAD_LAST, o.SMALL_STATES_NONE, head_bias=False)[1]
        assert bool(((logits.double() - bare.double() - c['head_b'].double()).abs() <= 4 * torch.finfo(dt).eps * (1 + logits.double().abs())).all())


@kernel_cases
def test_y_within_the_summation_order_bound(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    B, T, F, N, O = c['B'], c['T'], c['F'], c['N'], c['O']
    y = _head_forward(c, o.SMALL_EDGE_HEAD_NODE, o.SMALL_STATES_NONE)[1]
    with torch.no_grad():
        ref = o.node_linear(c['H'].reshape(B * T, F, N), c['node_w'], c['node_b']).view(B, T, O, N)
    bound = 2.0 * F * torch.finfo(dt).eps * torch.einsum('of,btfn->bton', c['node_w'].double().abs(), c['H'].double().abs())
    err = (y.double() - ref.double()).abs()
    print('%s %s: max|y - node_linear| = %.3g, max err / bound = %.3g' % (shape, dt, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    if bias:                                               # |node_b| >= 1 is not silently dropped
        assert float(c['node_b'].abs().min()) >= 1.0
        bare = _head_forward(c, o.SMALL_EDGE_HEAD_NODE, o.SMALL_STATES_NONE, head_bias=False)[1]
        nb = c['node_b'].double().view(1, 1, O, 1)
        assert float((y - bare).abs().min()) >= 0.9
        assert bool(((y.double() - bare.double() - nb).abs() <= bound + 4 * torch.finfo(dt).eps * y.double().abs()).all())


LEAVES = ('X', 'h0', 'wA', 'wB', 'b', 'm_in', 'w_in', 'm_f', 'w_f', 'gi', 'gf')


def _grads(c, how, dx):
    """Gradients of every operand through a new one-node path ('last' / 'node') or through the existing _SmallEdgeCell fed the equivalent
    dH ('last_ref' / 'node_ref')."""
    o = ops()
    leaf = {k: (c[k].clone().requires_grad_(k != 'X' or dx) if c[k] is not None else None) for k in LEAVES}
    args = _cell_args(c, leaf)
    if how == 'last':
        o.small_edge_cell_classify(*args, c['head_w'], c['head_b'], leaf['gi'], leaf['gf']).backward(c['dlogits'])
    elif how == 'node':
        o.small_edge_cell_regress(*args, c['node_w'], c['node_b'], leaf['gi'], leaf['gf']).backward(c['dY'])
    else:
        if how == 'last_ref':
            dH = torch.zeros_like(c['H'])
            dH[:, -1] = torch.einsum('bc,ci->bi', c['dlogits'], c['head_w']).view(c['B'], c['F'], c['N'])
        else:
            dH = torch.einsum('of,bton->btfn', c['node_w'], c['dY']).contiguous()
        o.small_edge_cell_train(*args, leaf['gi'], leaf['gf']).backward(dH)
    return {k: v.grad for k, v in leaf.items() if v is not None and v.requires_grad}


@pytest.mark.parametrize('kind', ['last', 'node'])
@kernel_cases
def test_backward_equals_the_existing_backward_bit_for_bit(shape, dt, bias, gates, kind, spy):
    c = _case(shape, dt, bias, gates)
    if kind == 'last':                                      # exact in either dtype: small dyadic rationals
        exact = torch.einsum('bc,ci->bi', c['dlogits'].double(), c['head_w'].double())
        assert torch.equal(torch.einsum('bc,ci->bi', c['dlogits'], c['head_w']).double(), exact) and float(exact.abs().max()) <= 2 * c['C']
    else:
        exact = torch.einsum('of,bton->btfn', c['node_w'].double(), c['dY'].double())
        assert torch.equal(torch.einsum('of,bton->btfn', c['node_w'], c['dY']).double(), exact) and float(exact.abs().max()) <= 2 * c['O']
    for dx in (False, True):
        before = _grads(c, kind + '_ref', dx)
        spy.calls.clear()
        new = _grads(c, kind, dx)
        assert spy.calls[FWD_HEAD] == 1 and spy.calls[BWD_HEAD] == 1 and spy.calls[E_FWD] == 0 and spy.calls[E_BWD] == 0 \
            and spy.calls[E_DX] == 0, dict(spy.calls)
        again = _grads(c, kind, dx)
        spy.calls.clear()
        ref = _grads(c, kind + '_ref', dx)                 # the existing entries, called before and after the new path: unchanged bits
        assert spy.calls[BWD_HEAD] == 0 and spy.calls[E_DX if dx else E_BWD] == 1 and spy.calls[E_FWD] == 1, dict(spy.calls)
        want = {'h0', 'wA', 'wB', 'm_in', 'w_in', 'm_f', 'w_f'} | ({'X'} if dx else set()) | ({'b'} if c['b'] is not None else set()) | \
            ({'gi', 'gf'} if gates != 'none' else set())
        assert set(new) == want and set(ref) == want
        for k in sorted(want):
            assert new[k] is not None and new[k].shape == ref[k].shape and bool(torch.isfinite(new[k]).all()), k
            assert _spread(ref[k]), k
            assert torch.equal(new[k], ref[k]), (k, dx, float((new[k] - ref[k]).abs().max()))
            assert torch.equal(new[k], again[k]), (k, dx, 'two runs differ')
            assert torch.equal(before[k], ref[k]), (k, dx, 'the existing entry changed its bits')


def test_head_parameter_gradients_are_the_library_products(spy):
    o, c = ops(), _case('quake59', F64, True, 'time')
    hw, hb = c['head_w'].clone().requires_grad_(True), c['head_b'].clone().requires_grad_(True)
    o.small_edge_cell_classify(*_cell_args(c), hw, hb, c['gi'], c['gf']).backward(c['dlogits'])
    assert spy.calls[BWD_HEAD] == 1 and spy.calls[E_BWD] == 0 and spy.calls[E_DX] == 0, dict(spy.calls)
    want = c['dlogits'].t() @ c['H_last'].reshape(c['B'], -1)
    assert float((hw.grad - want).abs().max()) <= 1e-12 * float(want.abs().max()) and torch.equal(hb.grad, c['dlogits'].sum(0))
    nw, nb = c['node_w'].clone().requires_grad_(True), c['node_b'].clone().requires_grad_(True)
    spy.calls.clear()
    o.small_edge_cell_regress(*_cell_args(c), nw, nb, c['gi'], c['gf']).backward(c['dY'])
    assert spy.calls[BWD_HEAD] == 1 and spy.calls[NL_BWD] == 1 and spy.calls[NL_FWD] == 0 and spy.calls[E_BWD] == 0, dict(spy.calls)
    want = torch.einsum('bton,btfn->of', c['dY'], c['H'])
    assert _spread(nw.grad) and float((nw.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(nb.grad, c['dY'].sum((0, 1, 3)))


# ------------------------------------------------------------------------------------------------------------------ model level
def _cls_model(tg, dims=(11,)):
    torch.manual_seed(59)
    return archit().GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, list(dims), _adj59(), True, time_gating=tg,
                                                spatial_gating='edge').double()


def _reg_model(tg, dims=(1,), mlp='multipMlp', S=None, F=20, K=5):
    torch.manual_seed(50)
    S = gso_sbm50()[0] if S is None else S
    return archit().GatedGCRNNforRegression(1, F, K, K, torch.tanh, torch.nn.ReLU, list(dims), S, True, time_gating=tg,
                                            spatial_gating='edge', mlpType=mlp).double()


def _model_inputs(kind, T=None, B=None):
    N, T0, B0, seed = (59, 20, 3, 59) if kind == 'cls' else (50, 5, 4, 50)
    T, B = T or T0, B or B0
    rng = np.random.default_rng(seed + T)
    return rng.standard_normal((B, T, 1, N)), 0.5 * np.tanh(rng.standard_normal((B, 20, N)))


def _dev(a, dt):
    return torch.tensor(a, dtype=dt, device=DEV)


def _new_path_only(spy, kind, forwards, backwards):
    c = spy.calls
    assert c[FWD_HEAD] == forwards and c[BWD_HEAD] == backwards, dict(c)
    assert c['small_edge_cell_classify' if kind == 'cls' else 'small_edge_cell_regress'] == forwards, dict(c)
    assert c[E_FWD] == 0 and c[E_BWD] == 0 and c[E_DX] == 0 and c[NL_FWD] == 0 and c['node_linear'] == 0, dict(c)
    assert c['small_edge_cell_forward'] == 0 and c['small_edge_cell_train'] == 0, dict(c)


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('tg', [False, True], ids=['edge', 'time+edge'])
@pytest.mark.parametrize('kind,dims', [('cls', (11,)), ('reg', (1,)), ('reg', (3,))])
def test_models_against_the_oracle(kind, dims, tg, dt, spy, monkeypatch):
    m = _cls_model(tg, dims) if kind == 'cls' else _reg_model(tg, dims)
    S = _adj59()[None] if kind == 'cls' else gso_sbm50()
    x, h0 = _model_inputs(kind)
    params = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    if kind == 'cls':
        want = orc.gated_gcrnn_classification(params, S, x, h0, time_gating=tg, spatial_gating='edge')
    else:
        want = orc.gated_gcrnn_regression(params, S, x, h0, time_gating=tg, spatial_gating='edge', mlp_type='multipMlp')
    m = m.to(DEV).to(dt)
    _switch_on(monkeypatch, kind, dt)
    with torch.no_grad():
        y = m(_dev(x, dt), _dev(h0, dt))
    _new_path_only(spy, kind, 1, 0)
    assert tuple(y.shape) == want.shape
    err = float(np.max(np.abs(y.double().cpu().numpy() - want)))
    print('%s %s time_gating=%s %s: max-abs %.3e' % (kind, dims, tg, dt, err))
    assert err <= TOL[dt]


def _torch_model(m, kind, tg, S, x, h0, loss, target, x_grad=False, stacked=False):
    """(y, {parameter name / 'h0' / 'x': gradient}) of the model under CPU fp64 autograd: oracle/torch_reference.ggcrnn_cell plus a torch head."""
    params = {k: v.detach().clone().requires_grad_() for k, v in m.state_dict().items()}
    cell = {k[len('stateGCRNN.'):]: v for k, v in params.items() if k.startswith('stateGCRNN.')}
    xt, ht = torch.tensor(x, requires_grad=x_grad), torch.tensor(h0, requires_grad=True)
    xin = xt * 1.0
    if stacked:                                            # the first call's output, squeezed to one feature, feeds the second
        xin = tr.ggcrnn_cell(cell, torch.tensor(S), xin, ht, time_gating=tg, spatial_gating='edge').mean(dim=2, keepdim=True)
    H = tr.ggcrnn_cell(cell, torch.tensor(S), xin, ht, time_gating=tg, spatial_gating='edge')
    B, T, F, N = H.shape
    W, b = params['outputNN.0.weight'], params['outputNN.0.bias']
    if kind == 'cls':
        y = H[:, -1].reshape(B, F * N) @ W.t() + b
    else:
        y = (torch.einsum('of,btfn->bton', W, H) + b.view(1, 1, -1, 1)).reshape(B, T, -1).unsqueeze(2)
    _loss(y, torch.tensor(target), loss).backward()
    grads = {k: v.grad.detach() for k, v in params.items() if v.grad is not None}
    grads['h0'] = ht.grad.detach()
    if x_grad:
        grads['x'] = xt.grad.detach()
    return y.detach(), grads


def _loss(y, target, loss):
    return (y * target).sum() if loss == 'sum' else (y - target).abs().mean()


def _device_model(m, x, h0, loss, target, dt, x_grad=False, stacked=False):
    m = copy.deepcopy(m).to(DEV).to(dt)
    xd, hd = _dev(x, dt).requires_grad_(x_grad), _dev(h0, dt).requires_grad_()
    xin = xd
    if stacked:
        xin = m.stateGCRNN(xd, hd).mean(dim=2, keepdim=True)
    y = m(xin, hd)
    _loss(y, _dev(target, dt), loss).backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    grads['h0'] = hd.grad
    if x_grad:
        grads['x'] = xd.grad
    return y.detach(), grads


def _check_step(y, grads, yref, gref, dt, label):
    tol_y, tol_g = TOLS[dt]
    err = float((y.double().cpu() - yref).abs().max())
    print('%s %s: outputs max-abs %.3e' % (label, dt, err))
    assert err <= tol_y
    assert set(gref) <= set(grads), sorted(set(gref) - set(grads))
    for k in sorted(gref):
        big = float(gref[k].abs().max())
        assert big > 0, k
        e = float((grads[k].double().cpu() - gref[k]).abs().max()) / big
        print('%s %s: grad %-44s rel %.3e' % (label, dt, k, e))
        assert e <= tol_g, k


@functools.lru_cache(maxsize=None)
def _train_reference(kind, tg, loss, x_grad, stacked):
    m = _cls_model(tg) if kind == 'cls' else _reg_model(tg, (3,))
    S = _adj59()[None] if kind == 'cls' else gso_sbm50()
    x, h0 = _model_inputs(kind, T=4 if kind == 'cls' else 5, B=3)
    shape = (x.shape[0], 11) if kind == 'cls' else (x.shape[0], x.shape[1], 1, 3 * x.shape[3])
    target = np.random.default_rng(7).standard_normal(shape)
    yref, gref = _torch_model(m, kind, tg, S, x, h0, loss, target, x_grad, stacked)
    return m, x, h0, target, yref, gref


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('loss', ['sum', 'l1'])
@pytest.mark.parametrize('tg', [False, True], ids=['edge', 'time+edge'])
@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_training_step_against_the_torch_reference(kind, tg, loss, dt, spy, monkeypatch):
    m, x, h0, target, yref, gref = _train_reference(kind, tg, loss, False, False)
    _switch_on(monkeypatch, kind, dt)
    y, grads = _device_model(m, x, h0, loss, target, dt)
    _new_path_only(spy, kind, 1, 1)
    # the head's parameters, both attentions' mixer and weight and the time-gate sub-networks all receive gradients
    need = {'outputNN.0.weight', 'outputNN.0.bias', 'h0'} | {'stateGCRNN.%s_attention.%s' % (a, p) for a in ('input', 'forget')
                                                             for p in ('mixer', 'weight')}
    if tg:
        need |= {'stateGCRNN.GFL_in.weight_A', 'stateGCRNN.MLP_forget.0.weight'}
    assert need <= set(gref) and need <= set(grads), sorted(need - set(gref))
    _check_step(y, grads, yref, gref, dt, '%s tg=%s %s' % (kind, tg, loss))


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('stacked', [False, True], ids=['dx', 'stacked'])
@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_input_gradient_and_stacked_calls(kind, stacked, dt, spy, monkeypatch):
    m, x, h0, target, yref, gref = _train_reference(kind, True, 'sum', True, stacked)
    _switch_on(monkeypatch, kind, dt)
    monkeypatch.setenv('GCRNN_SMALL_EDGE_DX', '1')
    y, grads = _device_model(m, x, h0, 'sum', target, dt, x_grad=True, stacked=stacked)
    assert spy.calls[FWD_HEAD] == 1 and spy.calls[BWD_HEAD] == 1 and spy.calls[E_BWD] == 0, dict(spy.calls)
    assert spy.calls[E_DX] == (1 if stacked else 0) and spy.calls[E_FWD] == (1 if stacked else 0), dict(spy.calls)
    assert 'x' in gref and _spread(grads['x'])
    _check_step(y, grads, yref, gref, dt, '%s %s' % (kind, 'stacked' if stacked else 'dx'))


def _step(m, x, h0, target):
    m.zero_grad(set_to_none=True)
    y = m(x, h0)
    (y * target).sum().backward()
    return y.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_switch_and_off_switches(kind, spy, monkeypatch):
    m = (_cls_model(True) if kind == 'cls' else _reg_model(True)).to(DEV)
    x, h0 = (_dev(a, F64) for a in _model_inputs(kind, T=4))
    with torch.no_grad():
        target = torch.randn(m(x, h0).shape, generator=torch.Generator().manual_seed(3), dtype=F64).to(DEV)
    # unset: the two-module path, as the parent
    spy.calls.clear()
    with torch.no_grad():
        y_off = m(x, h0)
    assert spy.calls['small_edge_cell_forward'] == 1 and spy.calls[E_FWD] == 1 and spy.calls[FWD_HEAD] == 0, dict(spy.calls)
    assert spy.calls['node_linear'] == (1 if kind == 'reg' else 0), dict(spy.calls)
    spy.calls.clear()
    yt_off, g_off = _step(m, x, h0, target)
    assert spy.calls['small_edge_cell_train'] == 1 and spy.calls[E_BWD] == 1 and spy.calls[FWD_HEAD] == 0 and spy.calls[BWD_HEAD] == 0, dict(spy.calls)
    assert spy.calls['node_linear'] == (1 if kind == 'reg' else 0), dict(spy.calls)
    # set: one forward call per forward, one backward call per backward, none of the existing entries
    _switch_on(monkeypatch, kind, F64)
    spy.calls.clear()
    with torch.no_grad():
        y_on = m(x, h0)
    _new_path_only(spy, kind, 1, 0)
    spy.calls.clear()
    yt_on, g_on = _step(m, x, h0, target)
    _new_path_only(spy, kind, 1, 1)
    assert float((y_on - y_off).abs().max()) <= TOL[F64] and float((yt_on - yt_off).abs().max()) <= TOL[F64] and _spread(y_on)
    assert set(g_on) == set(g_off)
    for n in sorted(g_off):
        assert float((g_on[n] - g_off[n]).abs().max()) <= 1e-10 * float(g_off[n].abs().max()), n
    # each off-switch wins, and gives the bits of the unset switch (the composed path under GCRNN_NO_SMALL_EDGE has its own)
    for off in ('GCRNN_NO_SMALL_HEAD' if kind == 'cls' else 'GCRNN_NO_SMALL_NODE_HEAD', 'GCRNN_NO_SMALL_EDGE'):
        monkeypatch.setenv(off, '1')
        spy.calls.clear()
        with torch.no_grad():
            y = m(x, h0)
        yt, g = _step(m, x, h0, target)
        assert spy.calls[FWD_HEAD] == 0 and spy.calls[BWD_HEAD] == 0, (off, dict(spy.calls))
        if off != 'GCRNN_NO_SMALL_EDGE':
            assert torch.equal(y, y_off) and torch.equal(yt, yt_off) and all(torch.equal(g[n], g_off[n]) for n in g_off), off
        else:
            assert spy.calls[E_FWD] == 0 and float((y - y_off).abs().max()) <= 1e-9
        monkeypatch.delenv(off)
    if kind == 'reg':                                      # =1 leaves the fp64 per-node head on the two-module path (_small_edge_head_pays)
        monkeypatch.setenv(SWITCH, '1')
        spy.calls.clear()
        with torch.no_grad():
            y = m(x, h0)
        yt, g = _step(m, x, h0, target)
        assert spy.calls[FWD_HEAD] == 0 and spy.calls[BWD_HEAD] == 0 and spy.calls['node_linear'] == 2, dict(spy.calls)
        assert torch.equal(y, y_off) and torch.equal(yt, yt_off) and all(torch.equal(g[n], g_off[n]) for n in g_off)
        spy.calls.clear()
        m32 = copy.deepcopy(m).float()                     # ... and takes the fp32 one
        with torch.no_grad():
            m32(x.float(), h0.float())
        _new_path_only(spy, kind, 1, 0)
    monkeypatch.delenv(SWITCH)
    with torch.no_grad():
        assert torch.equal(m(x, h0), y_off)                # read at every call


def test_heads_that_do_not_qualify_fall_back(spy, monkeypatch):
    def same_with_the_switch(m, x, h0, dt=F64, inference_too=True):
        """The model's training step (and its inference) does not take the new path, and the switch changes nothing about what it gives."""
        x, h0 = _dev(x, dt), _dev(h0, dt)
        monkeypatch.delenv(SWITCH, raising=False)
        with torch.no_grad():
            target = torch.ones_like(m(x, h0))
        y, g = _step(m, x, h0, target)
        monkeypatch.setenv(SWITCH, 'all')
        spy.calls.clear()
        y2, g2 = _step(m, x, h0, target)
        assert spy.calls[FWD_HEAD] == 0 and spy.calls[BWD_HEAD] == 0, dict(spy.calls)
        with torch.no_grad():
            m(x, h0)
        assert spy.calls[FWD_HEAD] == (0 if inference_too else 1) and spy.calls[BWD_HEAD] == 0, dict(spy.calls)
        monkeypatch.delenv(SWITCH)
        assert torch.equal(y, y2) and set(g) == set(g2) and all(torch.equal(g[n], g2[n]) for n in g2)
    xc, hc = _model_inputs('cls', T=3)
    xr, hr = _model_inputs('reg', T=3)
    same_with_the_switch(_cls_model(False, dims=(16, 11)).to(DEV), xc, hc)                          # two Linear layers
    same_with_the_switch(_reg_model(False, dims=(16, 1)).to(DEV), xr, hr)
    same_with_the_switch(_reg_model(False, dims=(50,), mlp='oneMlp').to(DEV), xr, hr)                # one MLP over all nodes
    half = _reg_model(False).to(DEV)                                                                # fp32 states meeting an fp64 head
    half.stateGCRNN.float()
    same_with_the_switch(half, xr, hr, F32)
    same_with_the_switch(_reg_model(False, dims=(9,)).to(DEV), xr, hr)                               # O = 9
    from test_small_edge import gso_rand80                                                         # fp64 training the backward refuses
    rng = np.random.default_rng(80)
    big = _reg_model(False, S=gso_rand80()[0], F=32, K=3).to(DEV)
    x80, h80 = rng.standard_normal((2, 3, 1, 80)), 0.5 * np.tanh(rng.standard_normal((2, 32, 80)))
    same_with_the_switch(big, x80, h80, inference_too=False)                                        # (its inference fits and takes the new path)


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_neither_the_states_nor_dh_are_allocated(spy, monkeypatch):
    """adj59, F = 20, T = 50, B = 8, fp64: states = B T F N 8 bytes. Regression inference: H is gone (Ya stays), so the peak with the switch is
    lower by at least 0.9 states. Classification training step: the zero-filled dH is gone, lower by at least 0.9 states."""
    B, T, F, N = 8, 50, 20, 59
    states = B * T * F * N * 8
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, T, 1, N, generator=gen, dtype=F64).to(DEV)
    h0 = (0.3 * torch.randn(B, F, N, generator=gen, dtype=F64)).to(DEV)
    torch.manual_seed(59)
    reg = archit().GatedGCRNNforRegression(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [1], _adj59(), True, time_gating=False,
                                           spatial_gating='edge', mlpType='multipMlp').double().to(DEV)
    cls = _cls_model(False).to(DEV)

    def infer():
        with torch.no_grad():
            return reg(x, h0)

    def train():
        cls.zero_grad(set_to_none=True)
        y = cls(x, h0)
        y.sum().backward()
        return y.detach()
    for name, fn, kind, bwd in (('regression inference', infer, 'reg', 0), ('classification training', train, 'cls', 1)):
        seen = {}
        for on in (False, True):
            if on:
                _switch_on(monkeypatch, kind, F64)
            else:
                monkeypatch.delenv(SWITCH, raising=False)
            fn()                                           # warm-up: plans, allocator pools
            spy.calls.clear()
            seen[on], out = _peak(fn)
            if on:
                _new_path_only(spy, kind, 1, bwd)
            else:
                assert spy.calls[FWD_HEAD] == 0 and spy.calls[E_FWD] == 1, dict(spy.calls)
            del out
        print('%s: peak above baseline %.2f MB with the switch, %.2f MB without; states %.2f MB'
              % (name, seen[True] / 1e6, seen[False] / 1e6, states / 1e6))
        assert seen[False] - seen[True] >= 0.9 * states, name


@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_inference_captures_under_cuda_graph(kind, spy, monkeypatch):
    _switch_on(monkeypatch, kind, F32)
    m = (_cls_model(True) if kind == 'cls' else _reg_model(True)).to(DEV).float()
    x, h0 = (_dev(a, F32) for a in _model_inputs(kind, T=4))
    with torch.no_grad():
        want = m(x, h0)                                    # eager (and warm-up: the graph's plans are built here)
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            m(x, h0)
        torch.cuda.current_stream(DEV).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            yc = m(x, h0)
        yc.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(yc, want) and _spread(want)
    _new_path_only(spy, kind, 3, 0)
    del g


def test_graphed_train_step_replays_the_eager_step(spy, monkeypatch):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import GraphedTrainStep, train_step
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    _switch_on(monkeypatch, 'reg', F64)
    me = _reg_model(True).to(DEV)
    mg = copy.deepcopy(me)
    gen = torch.Generator().manual_seed(105)
    x = torch.randn(4, 5, 1, 50, generator=gen, dtype=F64).to(DEV)
    y = torch.randn(4, 5, 1, 50, generator=gen, dtype=F64).to(DEV)
    oe = optim.make_trainer('ADAM', me.parameters(), 1e-3, 0.9, 0.999, flat=True)
    og = optim.make_trainer('ADAM', mg.parameters(), 1e-3, 0.9, 0.999, flat=True)
    stepper = GraphedTrainStep(mg, batchTimeL1Loss, og, x, y, 20)                  # three eager warm-up steps, then the capture
    assert stepper.captured
    assert spy.calls[BWD_HEAD] == 4 and spy.calls[FWD_HEAD] == 4 and spy.calls[E_BWD] == 0 and spy.calls[E_FWD] == 0 \
        and spy.calls['node_linear'] == 0, dict(spy.calls)
    for _ in range(3):
        train_step(me, batchTimeL1Loss, oe, x, y, 20)
    for it in range(2):
        xb, yb = torch.roll(x, it + 1, dims=0), torch.roll(y, it + 1, dims=0)      # fresh inputs every replay
        loss_e, yhat_e = train_step(me, batchTimeL1Loss, oe, xb, yb, 20)
        loss_g, yhat_g = stepper(xb, yb)
        assert torch.equal(loss_e, loss_g) and torch.equal(yhat_e, yhat_g), it
        assert all(torch.equal(a, b) for a, b in zip(me.parameters(), mg.parameters())), it


@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_independent_of_what_the_work_buffers_held(kind, monkeypatch):
    from poison import assert_independent_of_workspace
    _switch_on(monkeypatch, kind, F64)

    def build_and_run():
        m = (_cls_model(True) if kind == 'cls' else _reg_model(True, (3,))).to(DEV)
        x, h0 = (_dev(a, F64) for a in _model_inputs(kind, T=3))
        hd = h0.clone().requires_grad_()
        with torch.no_grad():
            out = {'inference': m(x, h0)}
        y = m(x, hd)
        y.square().sum().backward()
        out['y'] = y.detach()
        out['h0.grad'] = hd.grad
        out.update({n: p.grad for n, p in m.named_parameters() if p.grad is not None})
        return out
    runs = assert_independent_of_workspace(build_and_run)
    assert _spread(runs['zero']['inference']) and len(runs['zero']) > 10


@pytest.mark.parametrize('kind', ['cls', 'reg'])
def test_a_nan_stays_in_its_sequence_and_step(kind, monkeypatch):
    _switch_on(monkeypatch, kind, F64)
    m = (_cls_model(True) if kind == 'cls' else _reg_model(True)).to(DEV)
    x, h0 = (_dev(a, F64) for a in _model_inputs(kind, T=5, B=3))
    bad = x.clone()
    bad[1, 2] = float('nan')
    with torch.no_grad():
        clean, y = m(x, h0), m(bad, h0)
    for b in (0, 2):
        assert torch.equal(y[b], clean[b]), b              # every other sequence: bit-identical
    if kind == 'cls':
        assert bool(torch.isnan(y[1]).all())
    else:
        assert torch.equal(y[1, :2], clean[1, :2])          # sequence 1 before step 2: untouched
        assert bool(torch.isnan(y[1, 2:]).all())           # ... and from step 2 on
