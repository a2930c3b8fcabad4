"""GPU (-m gpu): the regression model on small graphs with its per-node head inside the matrix-core kernels --
gcrnn_small_dense_forward_node_head (y_t from the state still in LDS, state-store modes) and gcrnn_small_dense_backward_node_head (BPTT that
forms dH_t = node_w^T dY_t itself), ops.small_cell_regress, GGCRNNCell.regress and GatedGCRNNforRegression.forward.

What is compared with what:
  states    the new entry point's all-states store against ops.small_cell_forward (same arithmetic: torch.equal); without a store it
            returns no H and the same y bits.
  y         against ops.node_linear(H, node_w, node_b) on the existing kernel's H. Two summation orders of F terms differ by at most
            2 F eps sum_f |node_w[o][f] h_t[f][n]| per element (each order is within F eps sum|.| of the exact sum); the test computes it.
  backward  dY are multiples of 1/4 in [-2, 2], node_w multiples of 1/8 in [-1, 1], none zero: every product and every sum of <= 3 of them is
            exact in fp32 and fp64, so dH = einsum('of,bton->btfn') is the same number however it is formed (a fused multiply-add rounds the
            same value), and the new backward must equal the existing _SmallCell backward fed that dH bit for bit.
  model     GCRNN_NO_SMALL_NODE_HEAD=1 (the two-module path) is the reference; fp64 gradients within 1e-10 of their maximum, fp32 gradients
            against the fp64 truth: at most twice the two-module fp32 path's own error plus 16 eps_fp32 max|g|.
Every GPU test uses a non-zero h0, a directed weighted GSO and seeded inputs. A counting wrapper shows which entry points ran."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_small_head import _CountingLib, _adj59, _gso, _spread, GATINGS

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FWD_NH, BWD_NH = 'gcrnn_small_dense_forward_node_head', 'gcrnn_small_dense_backward_node_head'
FWD_HEAD, BWD_HEAD = 'gcrnn_small_dense_forward_head', 'gcrnn_small_dense_backward_head'
D_FWD, D_BWD, D_DX = 'gcrnn_small_dense_forward', 'gcrnn_small_dense_backward', 'gcrnn_small_dense_backward_dx'
NL_FWD, NL_BWD = 'gcrnn_node_linear_forward', 'gcrnn_node_linear_backward'
SWITCH = 'GCRNN_NO_SMALL_NODE_HEAD'
F64, F32 = torch.float64, torch.float32


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
    for name in ('small_cell_forward', 'small_cell_train', 'small_cell_regress', 'node_linear'):
        def wrap(fn, name):
            def counted(*a, **kw):
                s.calls[name] += 1
                return fn(*a, **kw)
            return counted
        monkeypatch.setattr(o, name, wrap(getattr(o, name), name))
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    return s


def _new_path_only(spy, backward):
    c = spy.calls
    assert c[FWD_NH] >= 1 and c['small_cell_regress'] >= 1, dict(c)
    assert (c[BWD_NH] >= 1) == bool(backward), dict(c)
    assert c['small_cell_forward'] == 0 and c['small_cell_train'] == 0 and c['node_linear'] == 0, dict(c)
    # (the head's own parameter gradients are glue: node_linear's slot kernel with dh = NULL, once per backward and only there)
    assert c[D_FWD] == 0 and c[D_BWD] == 0 and c[D_DX] == 0 and c[NL_FWD] == 0 and c[NL_BWD] == (c[BWD_NH] if backward else 0), dict(c)


def _old_path_only(spy):
    c = spy.calls
    assert c['small_cell_regress'] == 0 and c[FWD_NH] == 0 and c[BWD_NH] == 0, dict(c)
    assert c['small_cell_forward'] + c['small_cell_train'] >= 1, dict(c)


def _bound(H, w):
    """2 F eps sum_f |w[o][f] h[..][f][n]| per output, in fp64. H [..][F][N], w [O][F] -> [..][O][N]."""
    F = w.shape[1]
    return 2.0 * F * torch.finfo(w.dtype).eps * torch.einsum('of,...fn->...on', w.double().abs(), H.double().abs())


# ------------------------------------------------------------------------------------------------------------------ kernel level
#          N, G,  F, Kin, Kst, T, B, O
SHAPES = {'quake59': (59, 1, 20, 4, 4, 3, 3, 1),           # N no multiple of 4 or 16; F spans two row tiles
          'exact16': (16, 2, 16, 2, 3, 2, 2, 3),           # exact tiles, Kin != Kst
          't1n17': (17, 1, 5, 3, 2, 1, 1, 3),              # T = 1: the only y is the one behind the loop; one column past a tile
          'five80': (80, 1, 20, 5, 5, 4, 2, 1),            # the k-step driver's graph size: five column tiles
          'two130': (130, 1, 20, 2, 2, 2, 2, 1)}           # fp32 only: 18 output tiles, the two-accumulator instantiation
CASES = [(s, dt) for s in ('quake59', 'exact16', 't1n17', 'five80') for dt in (F64, F32)] + [('two130', F32)]


def kernel_cases(fn):
    """Every shape and dtype, with and without bias (the cell's and the head's), with no gates, [T][B] gates and [B][T][N] gates."""
    fn = pytest.mark.parametrize('shape,dt', CASES, ids=['%s-%s' % (s, 'f64' if dt == F64 else 'f32') for s, dt in CASES])(fn)
    fn = pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])(fn)
    return pytest.mark.parametrize('gates', ['none', 'time', 'node'])(fn)


@functools.lru_cache(maxsize=None)
def _case(shape, dt, bias, gates):
    """Seeded operands of one kernel-level case on the device, and (computed once, never written again) the existing kernel's states."""
    from gated_gcrnns_amd.graph import GraphOperator
    N, G, F, Kin, Kst, T, B, O = SHAPES[shape]
    gen = torch.Generator().manual_seed(11 * N + 3 * T + B)

    def r(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    def u(*s):
        return torch.rand(*s, generator=gen, dtype=F64)

    def q(lo, hi, step, *s):                               # multiples of 1 / step in [lo, hi], none of them zero
        v = torch.randint(int(lo * step), int(hi * step) + 1, s, generator=gen).double()
        return torch.where(v == 0, torch.ones_like(v), v) / step
    c = dict(N=N, G=G, F=F, Kin=Kin, Kst=Kst, T=T, B=B, O=O, dt=dt)
    c['graph'] = GraphOperator(_gso(N)[None], device=DEV)
    t = dict(X=r(B, T, G, N), h0=0.5 * r(B, F, N), wA=(2 * u(F, 1, Kin, G) - 1) / np.sqrt(G * Kin), wB=(2 * u(F, 1, Kst, F) - 1) / np.sqrt(F * Kst),
             b=0.2 * r(F, 1), node_w=q(-1, 1, 8, O, F), node_b=(0.5 + u(O)) * torch.where(u(O) < 0.5, -1.0, 1.0), dY=q(-2, 2, 4, B, T, O, N),
             gi=0.1 + 0.8 * u(*((T, B) if gates == 'time' else (B, T, N))), gf=0.1 + 0.8 * u(*((T, B) if gates == 'time' else (B, T, N))))
    for k, v in t.items():
        c[k] = v.to(DEV).to(dt)
    if not bias:
        c['b'] = c['node_b'] = None
    if gates == 'none':
        c['gi'] = c['gf'] = None
    assert float(c['h0'].abs().min()) > 0
    # never skipped on a no: the shapes were chosen inside the kernels' envelope
    assert ops().small_dense_supported(N, G, F, Kin, Kst, dt, backward=True, gated=c['gi'] is not None)
    assert ops().small_node_head_supported(N, G, F, Kin, Kst, O, dt, False, c['gi'] is not None), shape
    assert ops().small_node_head_supported(N, G, F, Kin, Kst, O, dt, True, c['gi'] is not None, dx=True), shape
    assert ops().node_linear_supported(F, O, dt, N, dt)
    with torch.no_grad():
        c['H'] = ops().small_cell_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], c['gi'], c['gf'])
    return c


def _head_forward(c, store, head=True):
    o = ops()
    return o._small_node_head_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], c['node_w'], c['node_b'] if head else None,
                                      c['gi'], c['gf'], store)


@kernel_cases
def test_state_store_keeps_the_existing_bits(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    H_all, y_all = _head_forward(c, o.SMALL_STATES_ALL)
    H_none, y_none = _head_forward(c, o.SMALL_STATES_NONE)
    assert _spread(c['H']) and bool(torch.isfinite(c['H']).all())
    assert tuple(H_all.shape) == (c['B'], c['T'], c['F'], c['N']) and torch.equal(H_all, c['H'])
    assert H_none is None
    assert tuple(y_all.shape) == (c['B'], c['T'], c['O'], c['N']) and torch.equal(y_all, y_none)      # y does not depend on what is stored
    assert torch.equal(y_none, _head_forward(c, o.SMALL_STATES_NONE)[1])                              # fixed order: two runs, the same bits


@kernel_cases
def test_y_within_the_summation_order_bound(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    B, T, F, N, O = c['B'], c['T'], c['F'], c['N'], c['O']
    y = _head_forward(c, o.SMALL_STATES_NONE)[1]
    with torch.no_grad():
        ref = o.node_linear(c['H'].reshape(B * T, F, N), c['node_w'], c['node_b']).view(B, T, O, N)
    bound = _bound(c['H'], c['node_w'])
    err = (y.double() - ref.double()).abs()
    print('%s %s: max|y - node_linear| = %.3g, smallest bound %.3g, max err / bound = %.3g'
          % (shape, dt, float(err.max()), float(bound.min()), float((err / bound).max())))
    assert tuple(y.shape) == (B, T, O, N) and _spread(y) and bool(torch.isfinite(y).all())
    assert bool((err <= bound).all())
    if bias:                                               # the bias is not silently dropped: without it every output moves by |node_b| >= 0.5
        bare = _head_forward(c, o.SMALL_STATES_NONE, head=False)[1]
        nb = c['node_b'].double().view(1, 1, O, 1)
        moved = (y.double() - bare.double() - nb).abs()
        assert float((y - bare).abs().min()) >= 0.4 and bool((moved <= bound + 4 * torch.finfo(dt).eps * y.double().abs()).all())


def _grads(c, new, dx):
    """Gradients of every operand through the new one-node path or through the existing _SmallCell fed the equivalent dH."""
    o = ops()
    leaf = {k: (c[k].clone().requires_grad_(k != 'X' or dx) if c[k] is not None else None) for k in ('X', 'h0', 'wA', 'wB', 'b', 'gi', 'gf')}
    if new:
        y = o.small_cell_regress(leaf['X'], leaf['h0'], leaf['wA'], leaf['wB'], leaf['b'], c['graph'], c['node_w'], c['node_b'], leaf['gi'], leaf['gf'])
        y.backward(c['dY'])
    else:
        H = o.small_cell_train(leaf['X'], leaf['h0'], leaf['wA'], leaf['wB'], leaf['b'], c['graph'], leaf['gi'], leaf['gf'])
        H.backward(torch.einsum('of,bton->btfn', c['node_w'], c['dY']).contiguous())
    return {k: v.grad for k, v in leaf.items() if v is not None and v.requires_grad}


@kernel_cases
def test_backward_from_dy_equals_the_existing_backward_bit_for_bit(shape, dt, bias, gates, spy):
    c = _case(shape, dt, bias, gates)
    dH = torch.einsum('of,bton->btfn', c['node_w'].double(), c['dY'].double())      # exact in either dtype: small dyadic rationals
    assert torch.equal(torch.einsum('of,bton->btfn', c['node_w'], c['dY']).double(), dH) and float(dH.abs().max()) <= 2 * c['O']
    for dx in (False, True):
        spy.calls.clear()
        new = _grads(c, True, dx)
        assert spy.calls[BWD_NH] == 1 and spy.calls[FWD_NH] == 1 and spy.calls[D_BWD] == 0 and spy.calls[D_DX] == 0 and spy.calls[D_FWD] == 0 \
            and spy.calls[BWD_HEAD] == 0, dict(spy.calls)
        again = _grads(c, True, dx)
        spy.calls.clear()
        ref = _grads(c, False, dx)
        assert spy.calls[BWD_NH] == 0 and spy.calls[D_DX if dx else D_BWD] == 1, dict(spy.calls)
        want = {'h0', 'wA', 'wB'} | ({'X'} if dx else set()) | ({'b'} if bias else set()) | ({'gi', 'gf'} if gates != 'none' else set())
        assert set(new) == want and set(ref) == want
        for k in sorted(want):
            assert new[k] is not None and ref[k] is not None and new[k].shape == ref[k].shape, k
            assert _spread(ref[k]) and _spread(new[k]) and bool(torch.isfinite(new[k]).all()), k
            assert torch.equal(new[k], ref[k]), (k, dx, float((new[k] - ref[k]).abs().max()))
            assert torch.equal(new[k], again[k]), (k, dx, 'two runs differ')


@pytest.mark.parametrize('shape', ['quake59', 'exact16'])
def test_head_parameter_gradients_are_the_library_product(shape, spy):
    """d node_w = sum_{b,t} dY_t H_t^T and d node_b = sums of dY: glue (node_linear's slot kernel with dh = NULL, no [B][T][F][N] temporary),
    compared with autograd through node_linear's expression on the same H.
    d node_b is compared exactly: dY are multiples of 1/4 in [-2, 2], so every partial sum of the B T N <= 531 of them is exact."""
    o, c = ops(), _case(shape, F64, True, 'time')
    nw, nb = c['node_w'].clone().requires_grad_(True), c['node_b'].clone().requires_grad_(True)
    o.small_cell_regress(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], nw, nb, c['gi'], c['gf']).backward(c['dY'])
    assert spy.calls[BWD_NH] == 1 and spy.calls[NL_BWD] == 1 and spy.calls[D_BWD] == 0 and spy.calls[D_DX] == 0, dict(spy.calls)
    nw2, nb2 = c['node_w'].clone().requires_grad_(True), c['node_b'].clone().requires_grad_(True)
    (torch.einsum('of,btfn->bton', nw2, c['H']) + nb2.view(1, 1, -1, 1)).backward(c['dY'])
    assert _spread(nw.grad) and float((nw.grad - nw2.grad).abs().max()) <= 1e-12 * float(nw2.grad.abs().max())
    assert torch.equal(nb.grad, c['dY'].sum((0, 1, 3))) and torch.equal(nb.grad, nb2.grad)


@pytest.mark.parametrize('gates', ['none', 'node'])
def test_the_existing_backward_entries_keep_their_bits(gates):
    """gcrnn_small_dense_backward_head and gcrnn_small_dense_backward, fed identical inputs before and after a call of the new path, give
    identical bits: the third upstream source did not disturb the other two."""
    o, c = ops(), _case('quake59', F64, True, gates)
    gen = torch.Generator().manual_seed(5)
    head_w = (torch.randint(1, 9, (4, c['F'] * c['N']), generator=gen).double() / 8).to(DEV)
    dlogits = (torch.randint(1, 9, (c['B'], 4), generator=gen).double() / 4).to(DEV)
    dH = torch.randn(c['B'], c['T'], c['F'], c['N'], generator=gen, dtype=F64).to(DEV)

    def old_entries():
        out = []
        for kind in ('head', 'dH'):
            leaf = {k: (c[k].clone().requires_grad_(True) if c[k] is not None else None) for k in ('X', 'h0', 'wA', 'wB', 'b', 'gi', 'gf')}
            args = (leaf['X'], leaf['h0'], leaf['wA'], leaf['wB'], leaf['b'], c['graph'])
            if kind == 'head':
                o.small_cell_classify(*args, head_w, None, leaf['gi'], leaf['gf']).backward(dlogits)
            else:
                o.small_cell_train(*args, leaf['gi'], leaf['gf']).backward(dH)
            out += [v.grad.clone() for v in leaf.values() if v is not None]
        return out
    before = old_entries()
    _grads(c, True, True)
    after = old_entries()
    assert len(before) == len(after) >= 10 and all(_spread(a) for a in before)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


# ------------------------------------------------------------------------------------------------------------------ model level
def _model(gating, dims=(1,), final=None, K=4, mlp='multipMlp'):
    tg, sg = GATINGS[gating]
    torch.manual_seed(59)
    m = archit().GatedGCRNNforRegression(1, 20, K, K, torch.tanh, torch.nn.ReLU, list(dims), _adj59(), True, tg, sg, mlpType=mlp,
                                         finalNonlinearity=final).double()
    with torch.no_grad():                                                          # gates away from 0.5
        for name, p in m.named_parameters():
            if '.MLP_' in name:
                p.mul_(6.0)
            elif '.GFL_node_' in name:
                p.mul_(3.0)
    return m


def _inputs(T, B=3, dt=F64, O=1):
    gen = torch.Generator().manual_seed(100 + T)
    x = torch.randn(B, T, 1, 59, generator=gen, dtype=F64)
    h0 = 0.3 * torch.randn(B, 20, 59, generator=gen, dtype=F64)
    dy = torch.randn(B, T, 1, O * 59, generator=gen, dtype=F64)
    return x.to(DEV).to(dt), h0.to(DEV).to(dt), dy.to(DEV).to(dt)


def _step(m, x, h0, dy):
    """zero_grad, forward, backward from a fixed upstream dy: (y, {parameter name: gradient})."""
    m.zero_grad(set_to_none=True)
    y = m(x, h0)
    y.backward(dy)
    return y.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _y_bound(m, x, h0):
    """The summation-order bound on y in the model's output shape B x T x 1 x (O N), from the two-module path's own states."""
    with torch.no_grad():
        H = m.stateGCRNN(x, h0)
    return _bound(H, m.outputNN[0].weight.detach()).reshape(x.shape[0], x.shape[1], 1, -1)


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('gating', list(GATINGS))
def test_model_fp64_matches_the_two_module_path(gating, T, spy, monkeypatch):
    m = _model(gating).to(DEV)
    x, h0, dy = _inputs(T)
    with torch.no_grad():
        y_new = m(x, h0)
    _new_path_only(spy, backward=False)
    spy.calls.clear()
    yn, gn = _step(m, x, h0, dy)
    _new_path_only(spy, backward=True)
    assert spy.calls[FWD_NH] == 1 and spy.calls[BWD_NH] == 1
    monkeypatch.setenv(SWITCH, '1')                                                # read at every forward: same module, other path
    spy.calls.clear()
    with torch.no_grad():
        y_old = m(x, h0)
    _old_path_only(spy)
    bound = _y_bound(m, x, h0)
    spy.calls.clear()
    yo, go = _step(m, x, h0, dy)
    _old_path_only(spy)
    assert spy.calls['node_linear'] == 1 and spy.calls[NL_BWD] == 1, dict(spy.calls)
    for a, b in ((y_new, y_old), (yn, yo)):
        err = (a - b).abs()
        print('%s T=%d: max|y - two-module| = %.3g (bound >= %.3g)' % (gating, T, float(err.max()), float(bound.min())))
        assert tuple(a.shape) == (3, T, 1, 59) == tuple(b.shape) and bool((err <= bound).all()) and _spread(a)
    assert set(gn) == set(go) and {'outputNN.0.weight', 'outputNN.0.bias', 'stateGCRNN.weight_A', 'stateGCRNN.weight_B', 'stateGCRNN.bias'} <= set(gn)
    assert len(gn) > 5 or gating == 'none'                                         # the gates' own parameters get theirs
    for n in sorted(go):
        big = float(go[n].abs().max())
        assert big > 0, n
        rel = float((gn[n] - go[n]).abs().max()) / big
        print('  %-40s %.3g' % (n, rel))
        assert rel <= 1e-10, (n, rel)


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('gating', list(GATINGS))
def test_model_fp32_no_further_from_the_fp64_truth(gating, T, spy, monkeypatch):
    m64 = _model(gating).to(DEV)
    m32 = copy.deepcopy(m64).float()
    x, h0, dy = _inputs(T)
    _, gn = _step(m32, x.float(), h0.float(), dy.float())
    _new_path_only(spy, backward=True)
    monkeypatch.setenv(SWITCH, '1')
    spy.calls.clear()
    _, go = _step(m32, x.float(), h0.float(), dy.float())
    _old_path_only(spy)
    _, truth = _step(m64, x, h0, dy)
    assert set(gn) == set(go) == set(truth)
    eps = torch.finfo(F32).eps
    for n in sorted(truth):
        g = truth[n]
        e_new, e_old = float((gn[n].double() - g).abs().max()), float((go[n].double() - g).abs().max())
        print('%s T=%d %-40s new %.3g two-module %.3g' % (gating, T, n, e_new, e_old))
        assert e_new <= 2 * e_old + 16 * eps * float(g.abs().max()), (n, e_new, e_old)


@pytest.mark.parametrize('name', ['none', 'time'])
@pytest.mark.parametrize('dt,tol', [(F64, 1e-10), (F32, 1e-4)])
def test_reference_fixtures_on_the_new_path(dt, tol, name, spy):
    g = load_golden('g5_reg_multipMlp_%s' % name)
    m = archit().GatedGCRNNforRegression(1, 20, 2, 2, torch.tanh, torch.nn.ReLU, [1], g['S'][0], True, time_gating=name == 'time',
                                         spatial_gating=None, mlpType='multipMlp').double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    m = m.to(DEV).to(dt)
    x, h0 = torch.tensor(g['x'], dtype=dt, device=DEV), torch.tensor(g['h0'], dtype=dt, device=DEV)
    ref = torch.tensor(g['y'], device=DEV)
    with torch.no_grad():
        y0 = m(x, h0)
    _new_path_only(spy, backward=False)
    spy.calls.clear()
    y1 = m(x, h0)                                                                  # grad enabled: the training forward (every state stored)
    _new_path_only(spy, backward=False)
    assert y1.requires_grad
    for y in (y0, y1):
        assert tuple(y.shape) == tuple(ref.shape)
        err = float((y.detach().double() - ref).abs().max())
        print('%s %s: max|y - reference| = %.3g' % (name, dt, err))
        assert err <= tol


def test_three_outputs_per_node(spy, monkeypatch):
    m = _model('time', dims=(3,)).to(DEV)
    x, h0, dy = _inputs(5, O=3)
    yn, gn = _step(m, x, h0, dy)
    _new_path_only(spy, backward=True)
    monkeypatch.setenv(SWITCH, '1')
    spy.calls.clear()
    yo, go = _step(m, x, h0, dy)
    _old_path_only(spy)
    assert tuple(yn.shape) == (3, 5, 1, 3 * 59) == tuple(yo.shape)
    assert bool(((yn - yo).abs() <= _y_bound(m, x, h0)).all()) and _spread(yn)
    for n in sorted(go):
        assert float((gn[n] - go[n]).abs().max()) <= 1e-10 * float(go[n].abs().max()), n


def test_heads_that_do_not_qualify_fall_back(spy, monkeypatch):
    x, h0, dy = _inputs(5)

    def same_with_the_switch(m, xx, hh, dd):
        """The model does not take the new path, and the switch changes nothing about what it gives."""
        monkeypatch.delenv(SWITCH, raising=False)
        spy.calls.clear()
        y, g = _step(m, xx, hh, dd)
        assert spy.calls['small_cell_regress'] == 0 and spy.calls[FWD_NH] == 0 and spy.calls[BWD_NH] == 0, dict(spy.calls)
        calls = dict(spy.calls)
        monkeypatch.setenv(SWITCH, '1')
        y2, g2 = _step(m, xx, hh, dd)
        monkeypatch.delenv(SWITCH)
        assert torch.equal(y, y2) and set(g) == set(g2) and all(torch.equal(g[n], g2[n]) for n in g2)
        return calls
    calls = same_with_the_switch(_model('time', dims=(16, 1)).to(DEV), x, h0, dy)                      # two Linear layers
    assert calls['small_cell_train'] == 1 and calls.get('node_linear', 0) == 0, calls
    one = _model('none', mlp='oneMlp', dims=(59,)).to(DEV)                                             # one MLP over all nodes
    calls = same_with_the_switch(one, x, h0, dy)
    assert calls['small_cell_train'] == 1, calls
    half = _model('none').to(DEV)                                                                      # fp32 states meeting an fp64 head
    half.stateGCRNN.float()
    calls = same_with_the_switch(half, x.float(), h0.float(), dy)
    assert calls['small_cell_train'] == 1, calls
    torch.manual_seed(59)
    edge = archit().GatedGCRNNforRegression(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [1], _adj59(), True, False, 'edge',
                                            mlpType='multipMlp').double().to(DEV)
    calls = same_with_the_switch(edge, x, h0, dy)
    assert calls.get('small_cell_train', 0) == 0 and calls['node_linear'] == 1, calls                  # the edge-gated cell, then the head
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')                                                      # the gather family keeps its two modules
    calls = same_with_the_switch(_model('none').to(DEV), x, h0, dy)
    assert calls['node_linear'] == 1 and calls.get(D_BWD, 0) == 0 and calls.get(D_FWD, 0) == 0, calls
    monkeypatch.delenv('GCRNN_SMALL_GATHER')
    # a final nonlinearity is applied on top of the fused y
    sig = _model('none', final=torch.nn.Sigmoid).to(DEV)
    spy.calls.clear()
    with torch.no_grad():
        p_new = sig(x, h0)
    _new_path_only(spy, backward=False)
    monkeypatch.setenv(SWITCH, '1')
    with torch.no_grad():
        p_old = sig(x, h0)
    assert tuple(p_new.shape) == (3, 5, 1, 59) == tuple(p_old.shape)
    assert float(p_new.min()) > 0 and float(p_new.max()) < 1 and _spread(p_new)
    assert bool(((p_new - p_old).abs() <= _y_bound(sig, x, h0)).all())             # sigmoid is 1/4-Lipschitz: y's bound holds


def test_graphed_train_step_replays_the_eager_step(spy):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import GraphedTrainStep, train_step
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    me = _model('time').to(DEV)
    mg = copy.deepcopy(me)
    x, _, y = _inputs(5, B=4)
    oe = optim.make_trainer('ADAM', me.parameters(), 1e-3, 0.9, 0.999, flat=True)
    og = optim.make_trainer('ADAM', mg.parameters(), 1e-3, 0.9, 0.999, flat=True)
    stepper = GraphedTrainStep(mg, batchTimeL1Loss, og, x, y, 20)                  # three eager warm-up steps, then the capture
    assert stepper.captured
    assert spy.calls[BWD_NH] == 4 and spy.calls[FWD_NH] == 4 and spy.calls[D_BWD] == 0 and spy.calls['small_cell_train'] == 0 \
        and spy.calls['node_linear'] == 0, dict(spy.calls)
    for _ in range(3):
        train_step(me, batchTimeL1Loss, oe, x, y, 20)
    for it in range(3):
        xb = torch.roll(x, it + 1, dims=0)                                         # fresh inputs every replay
        yb = torch.roll(y, it + 1, dims=0)
        loss_e, yhat_e = train_step(me, batchTimeL1Loss, oe, xb, yb, 20)
        loss_g, yhat_g = stepper(xb, yb)
        assert torch.equal(loss_e, loss_g) and torch.equal(yhat_e, yhat_g), it
        assert all(torch.equal(a, b) for a, b in zip(me.parameters(), mg.parameters())), it
    assert spy.calls[BWD_NH] == 4 + 6, dict(spy.calls)                             # replays launch without passing through Python


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_neither_the_states_nor_dh_are_allocated(spy, monkeypatch):
    """The capability: un-gated model, fp64, B = T = 64. states = B T F N 8 = 38.7 MB, y is states / 20.
    Inference under no_grad stores no state: the peak above the baseline is < states / 8 (y alone is states / 20); the two-module path holds
    H, so >= states. A training step holds H, y, dy, the slots (~3 %) and the bmm temporary (~2 %), ~1.15 x states by count, so < 1.5 x; the
    two-module path holds H and dH, so >= 2 x. The caps follow from these allocation counts; the observed figures are printed."""
    B, T, F, N = 64, 64, 20, 59
    states = B * T * F * N * 8
    m = _model('none').to(DEV)
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(B, T, 1, N, generator=gen, dtype=F64).to(DEV)
    h0 = (0.3 * torch.randn(B, F, N, generator=gen, dtype=F64)).to(DEV)
    dy = torch.randn(B, T, 1, N, generator=gen, dtype=F64).to(DEV)

    def infer():
        with torch.no_grad():
            return m(x, h0)

    def train():
        m.zero_grad(set_to_none=True)
        y = m(x, h0)
        y.backward(dy)
        return y.detach()
    seen = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv(SWITCH, '1')
        for name, fn in (('infer', infer), ('train', train)):
            fn()                                                                   # warm-up: the dense GSO, allocator pools
            spy.calls.clear()
            seen[name, off], out = _peak(fn)
            if off:
                _old_path_only(spy)
            else:
                _new_path_only(spy, backward=name == 'train')
            seen[name, off, 'y'] = out
            del out
            print('%s %s: peak above baseline %.2f MB = %.3f x states (%.2f MB)'
                  % (name, 'two-module' if off else 'new', seen[name, off] / 1e6, seen[name, off] / states, states / 1e6))
    assert seen['infer', False] < states / 8
    assert seen['infer', True] >= states
    assert seen['train', False] < 1.5 * states
    assert seen['train', True] >= 2 * states
    bound = _y_bound(m, x, h0)
    for name in ('infer', 'train'):
        assert bool(((seen[name, False, 'y'] - seen[name, True, 'y']).abs() <= bound).all()) and _spread(seen[name, False, 'y'])
