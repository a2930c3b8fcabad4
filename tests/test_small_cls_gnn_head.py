"""GPU (-m gpu): the classification model on small graphs with its one-layer Selection-GNN head (GraphFilter(F -> 1, K_o) + activation +
Linear(N -> C) on the last state) inside the matrix-core launches -- gcrnn_small_dense_forward_cls_gnn_head (the last state's hop levels,
the filter, v and the wave-per-class read-out behind the plain time loop; state-store modes), gcrnn_small_dense_backward_cls_gnn_head
(dv, dz, the dU chain and the carry tile seeded before the time loop; dU a side output), ops.small_cell_classify_gnn,
GGCRNNCell.classify_gnn and the gnn_head branch of GatedGCRNNforClassification.forward.

What is compared with what:
  states    the new entry point's all-states store against ops.small_cell_forward (same arithmetic: torch.equal); the last-state store is
            its last slice; without a store it returns no H and the same logits bits.
  logits    against torch.nn.functional.linear on ops.graph_filter_layer(h_T, w, b, graph, act) on the existing kernel's h_T: two summation
            orders of one polynomial. v: either is within m eps A_v of the exact pre-activation, m = K_o F + (K_o - 1) N the longest chain
            of additions and A_v[n] = |b| + sum_k sum_f |w[k][f]| (|h_T| |S|^k)[f][n], so dv = 2 m eps A_v (the activations are
            1-Lipschitz; tanh and sigmoid add 4 eps for their two evaluations). The read-out of N + 1 terms then gives
            |dlogit_c| <= sum_n |lin_w[c][n]| dv_n + 2 (N + 1) eps (|lin_b[c]| + sum_n |lin_w[c][n]| |v[n]|). A_v is computed in fp64.
  seeding   dlogits and lin_w are dyadic, so dv is exact in either precision: dU_0 against dv act'(V) in fp64 (exact for relu and the
            identity, 4 eps |dv| otherwise: 1 - v^2 and v (1 - v) may be contracted); dU_k against dU_0 (S^T)^k within
            2 k N eps (|dU_0| |S^T|^k); with a random dlogits and the identity, dU_0 = dv within 2 C eps sum_c |dlogits| |lin_w|.
  backward  the new entry's cell gradients against gcrnn_small_dense_backward(_dx) fed a dH that is zero except dH[:, T-1] =
            einsum('kf,bkn->bfn', head_w, dU), dU as the new entry returned it: one reordered sum of K_o terms, compared by the model-level
            rule (fp64 1e-10 of the maximum; fp32 against the fp64 truth of the same BPTT, e_new <= 2 e_old + 16 eps_fp32 max|g|); at
            K_o = 1 with the identity (dyadic operands: single exact products) bit for bit.
  model     GCRNN_NO_SMALL_CLS_GNN_HEAD=1 (the two-module path) is the reference; fp64 within 1e-10 of the maximum, fp32 against the fp64
            truth by the same rule.
Every GPU test uses a non-zero h0, a directed weighted GSO and seeded inputs. A counting wrapper shows which entry points ran."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from poison import poisoned_allocations
from test_small_head import _CountingLib, _adj59, _gso, _spread, GATINGS
from test_small_gnn_head import _poly_abs
from test_small_node_head import _peak

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FWD_CLS, BWD_CLS = 'gcrnn_small_dense_forward_cls_gnn_head', 'gcrnn_small_dense_backward_cls_gnn_head'
GFL_FWD, GFL_BWD = 'gcrnn_graph_filter_layer_forward', 'gcrnn_graph_filter_layer_backward'
D_FWD, D_BWD, D_DX = 'gcrnn_small_dense_forward', 'gcrnn_small_dense_backward', 'gcrnn_small_dense_backward_dx'
D_FWD_HEAD, D_BWD_HEAD, D_BWD_NH = 'gcrnn_small_dense_forward_head', 'gcrnn_small_dense_backward_head', 'gcrnn_small_dense_backward_node_head'
ADJ = 'gcrnn_small_gnn_head_adjoint'
SWITCH, TAKE_ALL = 'GCRNN_NO_SMALL_CLS_GNN_HEAD', 'GCRNN_SMALL_CLS_GNN_HEAD'
F64, F32 = torch.float64, torch.float32
WRAPPERS = ('small_cell_forward', 'small_cell_train', 'small_cell_classify_gnn', 'graph_filter_layer')


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
    for name in WRAPPERS:
        def wrap(fn, name):
            def counted(*a, **kw):
                s.calls[name] += 1
                return fn(*a, **kw)
            return counted
        monkeypatch.setattr(o, name, wrap(getattr(o, name), name))
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    monkeypatch.setenv(TAKE_ALL, 'all')                    # also the rows that _small_cls_gnn_head_pays leaves to the two-module path
    return s


def _new_path_only(spy, backward):
    c = spy.calls
    assert c[FWD_CLS] >= 1 and c['small_cell_classify_gnn'] >= 1, dict(c)
    assert (c[BWD_CLS] >= 1) == bool(backward), dict(c)
    assert c['small_cell_forward'] == 0 and c['small_cell_train'] == 0 and c['graph_filter_layer'] == 0, dict(c)
    assert c[GFL_FWD] == 0 and c[GFL_BWD] == 0 and c[D_FWD] == 0 and c[D_BWD] == 0 and c[D_DX] == 0 and c[ADJ] == 0, dict(c)
    assert c[D_FWD_HEAD] == 0 and c[D_BWD_HEAD] == 0 and c[D_BWD_NH] == 0, dict(c)


def _old_path_only(spy):
    c = spy.calls
    assert c['small_cell_classify_gnn'] == 0 and c[FWD_CLS] == 0 and c[BWD_CLS] == 0, dict(c)
    assert c['small_cell_forward'] + c['small_cell_train'] >= 1 and c['graph_filter_layer'] >= 1 and c[GFL_FWD] >= 1, dict(c)


# ------------------------------------------------------------------------------------------------------------------ kernel level
#          N, G,  F, Kin, Kst, K_o, C, T, B
SHAPES = {'quake59': (59, 1, 20, 4, 4, 4, 11, 3, 3),       # the epicenter driver's own sizes
          'exact16': (16, 2, 16, 2, 3, 2, 1, 2, 2),        # no padding row, C = 1
          't1n17': (17, 1, 5, 3, 2, 5, 3, 1, 1),           # T = 1: the epilogue is all there is; K_o > K uses ZX
          'k1n17': (17, 1, 5, 2, 2, 1, 19, 2, 1),          # K_o = 1: no hop; C > 16: a second round of the class loop
          'five80': (80, 1, 20, 5, 5, 5, 5, 4, 2),         # the k-step driver's shape
          'two130': (130, 1, 20, 2, 2, 2, 2, 2, 2)}        # fp32 only: the two-accumulator instantiation
CASES = [(s, dt) for s in ('quake59', 'exact16', 't1n17', 'k1n17', 'five80') for dt in (F64, F32)] + [('two130', F32)]
ACTS = {'quake59': ('relu', 'tanh', None, 'sigmoid')}      # relu and tanh everywhere, the identity and sigmoid on one shape


def _acts(shape):
    return ACTS.get(shape, ('relu', 'tanh'))


def kernel_cases(fn):
    """Every shape and dtype, with and without biases (the cell's, the filter's and the Linear's), with no gates, [T][B] gates and
    [B][T][N] gates."""
    fn = pytest.mark.parametrize('shape,dt', CASES, ids=['%s-%s' % (s, 'f64' if dt == F64 else 'f32') for s, dt in CASES])(fn)
    fn = pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])(fn)
    return pytest.mark.parametrize('gates', ['none', 'time', 'node'])(fn)


@functools.lru_cache(maxsize=None)
def _case(shape, dt, bias, gates):
    """Seeded operands of one kernel-level case on the device, and (computed once, never written again) the existing kernel's states."""
    from gated_gcrnns_amd.graph import GraphOperator
    N, G, F, Kin, Kst, Ko, C, T, B = SHAPES[shape]
    gen = torch.Generator().manual_seed(17 * N + 3 * T + B + Ko + C)

    def r(*s):
        return torch.randn(*s, generator=gen, dtype=F64)

    def u(*s):
        return torch.rand(*s, generator=gen, dtype=F64)

    def q(lo, hi, step, *s):                               # multiples of 1 / step in [lo, hi], none of them zero
        v = torch.randint(int(lo * step), int(hi * step) + 1, s, generator=gen).double()
        return torch.where(v == 0, torch.ones_like(v), v) / step
    c = dict(N=N, G=G, F=F, Kin=Kin, Kst=Kst, Ko=Ko, C=C, T=T, B=B, dt=dt)
    S = _gso(N)
    c['graph'] = GraphOperator(S[None], device=DEV)
    c['S'] = torch.tensor(S, dtype=F64, device=DEV).to(dt)
    t = dict(X=r(B, T, G, N), h0=0.5 * r(B, F, N), wA=(2 * u(F, 1, Kin, G) - 1) / np.sqrt(G * Kin), wB=(2 * u(F, 1, Kst, F) - 1) / np.sqrt(F * Kst),
             b=0.2 * r(F, 1), head_w=q(-1, 1, 8, Ko, F), head_b=0.25 + 0.5 * u(1),      # (positive: relu leaves outputs alive on the smallest shapes too)
            
             lin_w=q(-1, 1, 8, C, N), lin_b=0.5 * r(C), dl=q(-2, 2, 4, B, C), dl_r=r(B, C),
             gi=0.1 + 0.8 * u(*((T, B) if gates == 'time' else (B, T, N))), gf=0.1 + 0.8 * u(*((T, B) if gates == 'time' else (B, T, N))))
    for k, v in t.items():
        c[k] = v.to(DEV).to(dt)
    if not bias:
        c['b'] = c['head_b'] = c['lin_b'] = None
    if gates == 'none':
        c['gi'] = c['gf'] = None
    assert float(c['h0'].abs().min()) > 0
    # never skipped on a no: the shapes were chosen inside the kernels' envelope
    assert ops().small_dense_supported(N, G, F, Kin, Kst, dt, backward=True, gated=c['gi'] is not None)
    assert ops().small_cls_gnn_head_supported(N, G, F, Kin, Kst, Ko, C, dt, False, c['gi'] is not None), shape
    assert ops().small_cls_gnn_head_supported(N, G, F, Kin, Kst, Ko, C, dt, True, c['gi'] is not None, dx=True), shape
    with torch.no_grad():
        c['H'] = ops().small_cell_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], c['gi'], c['gf'])
    return c


def _head_forward(c, store, act, V=None, biases=True):
    o = ops()
    return o._small_dense_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], c['gi'], c['gf'], store,
                                  ('cls_gnn', c['head_w'], c['head_b'] if biases else None, act, c['lin_w'], c['lin_b'] if biases else None, V))


def _new_v(c, act):
    V = torch.full((c['B'], c['N']), float('nan'), dtype=c['dt'], device=DEV)
    H, logits = _head_forward(c, ops().SMALL_STATES_ALL, act, V)
    return H, logits, V


@kernel_cases
def test_state_store_keeps_the_existing_bits(shape, dt, bias, gates, spy):
    o, c = ops(), _case(shape, dt, bias, gates)
    assert _spread(c['H']) and bool(torch.isfinite(c['H']).all())
    for act in _acts(shape):
        spy.calls.clear()
        H_all, lg_all, V = _new_v(c, act)
        H_last, lg_last = _head_forward(c, o.SMALL_STATES_LAST, act)
        H_none, lg_none = _head_forward(c, o.SMALL_STATES_NONE, act)
        assert spy.calls[FWD_CLS] == 3 and spy.calls[D_FWD] == 0 and spy.calls[GFL_FWD] == 0 and spy.calls[D_FWD_HEAD] == 0, dict(spy.calls)
        assert tuple(H_all.shape) == (c['B'], c['T'], c['F'], c['N']) and torch.equal(H_all, c['H'])
        assert tuple(H_last.shape) == (c['B'], 1, c['F'], c['N']) and torch.equal(H_last, c['H'][:, -1:])
        assert H_none is None
        assert tuple(lg_all.shape) == (c['B'], c['C']) and bool(torch.isfinite(lg_all).all()) and bool(torch.isfinite(V).all())
        assert torch.equal(lg_all, lg_none) and torch.equal(lg_all, lg_last)           # the logits do not depend on what is stored
        assert torch.equal(lg_none, _head_forward(c, o.SMALL_STATES_NONE, act)[1])     # fixed order: two runs, the same bits


def _v_bound(hT, w, b, S, act, dt):
    Ko, F = w.shape
    m = Ko * F + (Ko - 1) * hT.shape[-1]
    eps = torch.finfo(dt).eps
    return (2.0 * m * eps * _poly_abs(hT, w, b, S) + (4 * eps if act in ('tanh', 'sigmoid') else 0.0)).squeeze(-2)      # [B][N]


@kernel_cases
def test_logits_within_the_summation_order_bound(shape, dt, bias, gates):
    o, c = ops(), _case(shape, dt, bias, gates)
    B, F, N, Ko, C = c['B'], c['F'], c['N'], c['Ko'], c['C']
    eps = torch.finfo(dt).eps
    hT = c['H'][:, -1]
    for act in _acts(shape):
        _, lg, V = _new_v(c, act)
        with torch.no_grad():
            v_ref = o.graph_filter_layer(hT.contiguous(), c['head_w'].view(1, 1, Ko, F), c['head_b'].view(1, 1) if bias else None,
                                         c['graph'], act).view(B, N)
            ref = torch.nn.functional.linear(v_ref, c['lin_w'], c['lin_b'])
        dv = _v_bound(hT, c['head_w'], c['head_b'], c['S'], act, dt)
        lwa = c['lin_w'].double().abs()
        bound = dv @ lwa.t() + 2.0 * (N + 1) * eps * ((c['lin_b'].double().abs() if bias else 0.0) + v_ref.double().abs() @ lwa.t())
        ev, err = (V.double() - v_ref.double()).abs(), (lg.double() - ref.double()).abs()
        print('%s %s %s: max|v - graph_filter_layer| = %.3g (max / bound %.3g), max|logits - linear| = %.3g (max / bound %.3g)'
              % (shape, dt, act, float(ev.max()), float((ev / dv).max()), float(err.max()), float((err / bound).max())))
        assert tuple(lg.shape) == (B, C) and (_spread(lg) or B * C == 1) and bool(torch.isfinite(lg).all()) and _spread(V)
        assert bool((ev <= dv).all())
        assert bool((err <= bound).all())
        if bias and act is None:                           # the biases are not silently dropped
            bare = _head_forward(c, o.SMALL_STATES_NONE, act, biases=False)[1]
            want = c['lin_b'].double() + c['head_b'].double() * c['lin_w'].double().sum(1)
            assert bool(((lg.double() - bare.double() - want).abs() <= 2 * bound + 8 * eps * want.abs()).all())
            assert float((lg - bare).abs().max()) > 0


def _dact(V, act):
    return {None: torch.ones_like(V), 'relu': (V > 0).to(V.dtype), 'tanh': 1 - V * V, 'sigmoid': V * (1 - V)}[act]


def _bptt(c, seed, dx):
    """(dX, dh0, dwA, dwB, db, dgi, dgf) of one BPTT launch on the case's stored states."""
    return ops()._small_dense_bptt(c['X'], c['h0'], c['H'], c['wA'], c['wB'], c['b'], c['gi'], c['gf'], c['graph'], dx, True, seed)


def _new_bptt(c, act, V, dl, dx, fill=float('nan')):
    dU = torch.full((c['B'], c['Ko'], c['N']), fill, dtype=c['dt'], device=DEV)        # the kernel writes every element
    out = _bptt(c, ('dcls', dl, c['head_w'], c['lin_w'], V, act, dU), dx)
    return out, dU


@kernel_cases
def test_seeding(shape, dt, bias, gates, spy):
    c = _case(shape, dt, bias, gates)
    B, N, Ko, C = c['B'], c['N'], c['Ko'], c['C']
    eps = torch.finfo(dt).eps
    lw = c['lin_w'].double()
    for act in _acts(shape):
        V = _new_v(c, act)[2]
        spy.calls.clear()
        _, dU = _new_bptt(c, act, V, c['dl'], False)
        assert spy.calls[BWD_CLS] == 1 and spy.calls[ADJ] == 0 and spy.calls[D_BWD] == 0, dict(spy.calls)
        assert bool(torch.isfinite(dU).all()) and _spread(dU)
        assert torch.equal(dU, _new_bptt(c, act, V, c['dl'], True)[1])                  # two runs (and both DX variants), the same bits
        dv = c['dl'].double() @ lw                                                      # dyadic operands: exact in fp32 too
        dz = dv * _dact(V.double(), act)
        if act in ('tanh', 'sigmoid'):
            assert bool(((dU[:, 0].double() - dz).abs() <= 4 * eps * dv.abs()).all())
        else:
            assert torch.equal(dU[:, 0].double(), dz)
        z, za, St = dU[:, 0].double(), dU[:, 0].double().abs(), c['S'].double().t()
        for k in range(1, Ko):
            z, za = z @ St, za @ St.abs()
            err = (dU[:, k].double() - z).abs()
            assert bool((err <= 2 * k * N * eps * za).all()), (act, k, float(err.max()))
    # dv itself, from a dlogits that is not dyadic, through the identity
    V = _new_v(c, None)[2]
    _, dU = _new_bptt(c, None, V, c['dl_r'], False)
    dv = c['dl_r'].double() @ lw
    assert bool(((dU[:, 0].double() - dv).abs() <= 2 * C * eps * (c['dl_r'].double().abs() @ lw.abs())).all())


def _truth(c, dHT, dx):
    """The cell's gradients from torch autograd through its dense fp64 expression on the up-cast operands, fed dH_T on the last state:
    the fp64 truth of an fp32 case (every shape, also the one the fp64 kernels do not take)."""
    leaf = {k: (c[k].double().clone().requires_grad_(k != 'X' or dx) if c[k] is not None else None) for k in ('X', 'h0', 'wA', 'wB', 'b', 'gi', 'gf')}
    S, B, F = c['S'].double(), c['B'], c['F']
    bb = leaf['b'].view(1, F, 1) if leaf['b'] is not None else 0.0
    h = leaf['h0']
    for t in range(c['T']):
        ax, z = 0.0, leaf['X'][:, t]
        for k in range(c['Kin']):
            ax, z = ax + torch.einsum('fg,bgn->bfn', leaf['wA'][:, 0, k], z), z @ S
        bh, z = 0.0, h
        for k in range(c['Kst']):
            bh, z = bh + torch.einsum('fg,bgn->bfn', leaf['wB'][:, 0, k], z), z @ S
        if leaf['gi'] is None:
            pre = ax + bh + 2.0 * bb
        else:
            gi, gf = ((g[t].view(B, 1, 1) if g.dim() == 2 else g[:, t].unsqueeze(1)) for g in (leaf['gi'], leaf['gf']))
            pre = gi * (ax + bb) + gf * (bh + bb)
        h = torch.tanh(pre)
    h.backward(dHT.double())
    return {k: v.grad for k, v in leaf.items() if v is not None and v.requires_grad}


NAMES = ('X', 'h0', 'wA', 'wB', 'b', 'gi', 'gf')


def _named(c, out, dx):
    g = dict(zip(NAMES, out))
    return {k: v for k, v in g.items() if v is not None and (k != 'X' or dx)}


@kernel_cases
def test_backward_equals_the_existing_backward_fed_dh(shape, dt, bias, gates, spy):
    c = _case(shape, dt, bias, gates)
    eps32 = torch.finfo(F32).eps
    for act in _acts(shape) + ((None,) if c['Ko'] == 1 else ()):
        V = _new_v(c, act)[2]
        for dx in (False, True):
            spy.calls.clear()
            out, dU = _new_bptt(c, act, V, c['dl'], dx)
            assert spy.calls[BWD_CLS] == 1 and spy.calls[D_BWD] == 0 and spy.calls[D_DX] == 0 and spy.calls[ADJ] == 0, dict(spy.calls)
            new = _named(c, out, dx)
            again = _named(c, _new_bptt(c, act, V, c['dl'], dx)[0], dx)
            dH = torch.zeros_like(c['H'])
            dH[:, -1] = torch.einsum('kf,bkn->bfn', c['head_w'], dU)
            spy.calls.clear()
            ref = _named(c, _bptt(c, ('dH', dH, None), dx), dx)
            assert spy.calls[BWD_CLS] == 0 and spy.calls[D_DX if dx else D_BWD] == 1, dict(spy.calls)
            truth = _truth(c, dH[:, -1], dx) if dt == F32 else None
            want = {'h0', 'wA', 'wB'} | ({'X'} if dx else set()) | ({'b'} if bias else set()) | ({'gi', 'gf'} if gates != 'none' else set())
            assert set(new) == want and set(ref) == want
            for k in sorted(want):
                assert new[k].shape == ref[k].shape and _spread(ref[k]) and _spread(new[k]) and bool(torch.isfinite(new[k]).all()), k
                assert torch.equal(new[k], again[k]), (k, dx, 'two runs differ')
                if c['Ko'] == 1 and act is None:
                    # single products of dyadic dlogits, lin_w and head_w: exact, so dH_T is the same number however it is formed
                    assert torch.equal(new[k], ref[k]), (k, dx, float((new[k] - ref[k]).abs().max()))
                elif dt == F64:
                    big = float(ref[k].abs().max())
                    assert float((new[k] - ref[k]).abs().max()) <= 1e-10 * big, (k, dx, act)
                else:
                    g = truth[k]
                    e_new, e_old = float((new[k].double() - g).abs().max()), float((ref[k].double() - g).abs().max())
                    assert e_new <= 2 * e_old + 16 * eps32 * float(g.abs().max()), (k, dx, act, e_new, e_old)


@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
def test_existing_upstream_forms_keep_their_bits(dt, spy):
    """gcrnn_small_dense_backward, _backward_head and _backward_node_head, before and after calls of the new entry in this process: the
    same bits (a determinism check over repeated calls; the cross-tree evidence is the resource listing and the timing in DESIGN 4.16)."""
    c = _case('quake59', dt, True, 'time')
    B, T, F, N = c['B'], c['T'], c['F'], c['N']
    gen = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=F64).to(DEV).to(dt)
    dH, hw, dlg, nw, dY = mk(B, T, F, N), mk(11, F * N), mk(B, 11), mk(3, F), mk(B, T, 3, N)

    def run():
        out = {}
        for dx in (False, True):
            out['dH', dx] = _bptt(c, ('dH', dH, None), dx)
            out['dlogits', dx] = _bptt(c, ('dlogits', dlg, hw), dx)
            out['dY', dx] = _bptt(c, ('dY', dY, nw), dx)
        return out
    before = run()
    assert spy.calls[BWD_CLS] == 0 and spy.calls[D_BWD] == 1 and spy.calls[D_DX] == 1 and spy.calls[D_BWD_HEAD] == 2 and spy.calls[D_BWD_NH] == 2
    for act in ('relu', 'tanh'):
        V = _new_v(c, act)[2]
        for dx in (False, True):
            _new_bptt(c, act, V, c['dl'], dx)
    assert spy.calls[BWD_CLS] == 4
    after = run()
    for key in before:
        for a, b in zip(before[key], after[key]):
            assert (a is None) == (b is None)
            assert a is None or (torch.equal(a, b) and bool(torch.isfinite(a).all()) and _spread(a)), key


# ------------------------------------------------------------------------------------------------------------------ isolation, poison
def _classify_step(c, act, X, dl):
    """logits and every gradient of one training step through ops.small_cell_classify_gnn."""
    o = ops()
    names = ('X', 'h0', 'wA', 'wB', 'b', 'gi', 'gf', 'head_w', 'head_b', 'lin_w', 'lin_b')
    leaf = {k: (c[k] if k != 'X' else X) for k in names}
    leaf = {k: (v.clone().requires_grad_(True) if v is not None else None) for k, v in leaf.items()}
    lg = o.small_cell_classify_gnn(leaf['X'], leaf['h0'], leaf['wA'], leaf['wB'], leaf['b'], c['graph'], leaf['head_w'], leaf['head_b'],
                                   leaf['lin_w'], leaf['lin_b'], act, leaf['gi'], leaf['gf'])
    lg.backward(dl)
    out = {k: v.grad for k, v in leaf.items() if v is not None}
    out['logits'] = lg.detach()
    return out


@pytest.mark.parametrize('poison', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
def test_a_non_finite_input_stays_in_its_sequence(dt, poison, spy):
    """one workgroup per sequence, in both launches. With relu too: the NaN stays a NaN in its own sequence."""
    for gates in ('none', 'node'):
        c = _case('quake59', dt, True, gates)
        b0, t0, n0 = 1, 1, 5
        S = c['S']
        assert bool(S[n0].any()) and bool(S[:, n0].any())
        Xp = c['X'].clone()
        Xp[b0, t0, 0, n0] = poison
        others = [i for i in range(c['B']) if i != b0]
        for act in ('relu', 'tanh'):
            spy.calls.clear()
            clean = _classify_step(c, act, c['X'], c['dl'])
            dirty = _classify_step(c, act, Xp, c['dl'])
            assert spy.calls[FWD_CLS] == 2 and spy.calls[BWD_CLS] == 2, dict(spy.calls)
            assert all(bool(torch.isfinite(v).all()) for v in clean.values()) and _spread(clean['logits'])
            for k in ('logits', 'X', 'h0') + (('gi', 'gf') if gates == 'node' else ()):      # what has a row per sequence
                assert torch.equal(dirty[k][others], clean[k][others]), (gates, act, k)
            assert bool(torch.isnan(dirty['logits'][b0]).all()), (gates, act, dirty['logits'][b0])


@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
def test_poisoned_work_buffers_change_nothing(dt, spy):
    """H, V, dU, the logits and every slot buffer come from torch.empty; pre-filled with NaN they give the bits of zero-filled
    ones, in the training step and in the no-state inference launch."""
    o = ops()
    for shape, gates in (('quake59', 'time'), ('t1n17', 'node')):
        c = _case(shape, dt, True, gates)
        runs = {}
        for fill in ('zero', 'nan'):
            with poisoned_allocations(fill) as counter:
                out = _classify_step(c, 'tanh', c['X'], c['dl'])
                with torch.no_grad():
                    out['inference'] = o.small_cell_classify_gnn(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], c['head_w'],
                                                                 c['head_b'], c['lin_w'], c['lin_b'], 'tanh', c['gi'], c['gf'])
            assert counter.tensors > 4
            runs[fill] = out
        assert spy.calls[FWD_CLS] >= 4 and spy.calls[BWD_CLS] >= 2
        for k, v in runs['zero'].items():
            assert bool(torch.isfinite(v).all()) and torch.equal(v, runs['nan'][k]), (shape, k)
        assert torch.equal(runs['zero']['inference'], runs['zero']['logits'])
        # the buffers the caller hands over: V and dU
        for fill in (0.0, float('nan')):
            V = torch.full((c['B'], c['N']), fill, dtype=dt, device=DEV)
            _head_forward(c, o.SMALL_STATES_ALL, 'tanh', V)
            out, dU = _new_bptt(c, 'tanh', V, c['dl'], True, fill=fill)
            runs[fill != 0.0] = (V, dU) + tuple(out)
        for a, b in zip(runs[False], runs[True]):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_head_parameter_gradients(spy):
    """d head_w, d head_b, d lin_w, d lin_b (library products on dU, V and dlogits) against autograd through the dense fp64 expression of
    the head on the same last state."""
    for shape in ('quake59', 't1n17'):
        c = _case(shape, F64, True, 'time')
        for act in ('relu', 'tanh', 'sigmoid'):
            new = _classify_step(c, act, c['X'], c['dl_r'])
            p = {k: c[k].clone().requires_grad_(True) for k in ('head_w', 'head_b', 'lin_w', 'lin_b')}
            z, pre = c['H'][:, -1], p['head_b'].view(1, 1)
            for k in range(c['Ko']):
                pre = pre + torch.einsum('f,bfn->bn', p['head_w'][k], z)
                z = z @ c['S']
            v = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[act](pre)
            torch.nn.functional.linear(v, p['lin_w'], p['lin_b']).backward(c['dl_r'])
            for k, t in p.items():
                assert new[k].shape == t.grad.shape and _spread(new[k]), k
                assert float((new[k] - t.grad).abs().max()) <= 1e-11 * max(1.0, float(t.grad.abs().max())), (shape, act, k)


# ------------------------------------------------------------------------------------------------------------------ model level
def _model(gating, Ko=4, sigma2=torch.nn.ReLU, final=None, K=4, F_o=None, K_o=None, mlp=(11,)):
    import gated_gcrnns_amd.Utils.graphML as gml
    tg, sg = GATINGS[gating]
    F_o, K_o = list(F_o or [20, 1]), list(K_o or [Ko])
    torch.manual_seed(59)
    m = archit().GatedGCRNNforClassification(1, 20, K, K, torch.tanh, sigma2, list(mlp), _adj59(), True, tg, sg, final, F_o, K_o,
                                             [59] * len(K_o), gml.NoPool, [1] * len(K_o)).double()
    with torch.no_grad():                                                          # gates away from 0.5
        for name, p in m.named_parameters():
            if '.MLP_' in name:
                p.mul_(6.0)
            elif '.GFL_node_' in name:
                p.mul_(3.0)
            elif name == 'outputNN.0.GFL.0.bias':                                  # relu leaves outputs on both sides of its kink alive
                p.fill_(0.1)
    return m


def _inputs(T, B=3, dt=F64):
    gen = torch.Generator().manual_seed(300 + T)
    x = torch.randn(B, T, 1, 59, generator=gen, dtype=F64)
    h0 = 0.3 * torch.randn(B, 20, 59, generator=gen, dtype=F64)
    y = torch.randint(0, 11, (B,), generator=gen)
    return x.to(DEV).to(dt), h0.to(DEV).to(dt), y.to(DEV)


def _step(m, x, h0, y):
    """zero_grad, forward, cross-entropy, backward: (logits, {name: gradient}) with the gradients of x and h0 among them."""
    m.zero_grad(set_to_none=True)
    x, h0 = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    lg = m(x, h0)
    ops().cross_entropy(lg, y).backward()
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    g['x'], g['h0'] = x.grad, h0.grad
    return lg.detach(), g


HEAD_PARAMS = {'outputNN.0.GFL.0.weight', 'outputNN.0.GFL.0.bias', 'outputNN.0.MLP.0.weight', 'outputNN.0.MLP.0.bias'}
CELL_PARAMS = {'stateGCRNN.weight_A', 'stateGCRNN.weight_B', 'stateGCRNN.bias'}


@pytest.mark.parametrize('T', [1, 6])
@pytest.mark.parametrize('gating', list(GATINGS))
def test_model_fp64_matches_the_two_module_path(gating, T, spy, monkeypatch):
    m = _model(gating, Ko=5 if gating == 'time' else 4).to(DEV)                    # K_o = 5 > K = 4 on one gating
    x, h0, y = _inputs(T)
    with torch.no_grad():
        lg_new = m(x, h0)
    _new_path_only(spy, backward=False)
    assert spy.calls[FWD_CLS] == 1
    spy.calls.clear()
    lgn, gn = _step(m, x, h0, y)
    _new_path_only(spy, backward=True)
    assert spy.calls[FWD_CLS] == 1 and spy.calls[BWD_CLS] == 1
    monkeypatch.setenv(SWITCH, '1')                                                # read at every forward: same module, other path
    spy.calls.clear()
    with torch.no_grad():
        lg_old = m(x, h0)
    _old_path_only(spy)
    spy.calls.clear()
    lgo, go = _step(m, x, h0, y)
    _old_path_only(spy)
    assert spy.calls[GFL_BWD] == 1 and spy.calls[D_BWD] + spy.calls[D_DX] == 1, dict(spy.calls)
    for a, b in ((lg_new, lg_old), (lgn, lgo)):
        err = float((a - b).abs().max())
        print('%s T=%d: max|logits - two-module| = %.3g' % (gating, T, err))
        assert tuple(a.shape) == (3, 11) == tuple(b.shape) and _spread(a) and err <= 1e-10 * max(1.0, float(b.abs().max()))
    assert set(gn) == set(go) and (HEAD_PARAMS | CELL_PARAMS | {'x', 'h0'}) <= set(gn)
    assert len(gn) > 9 or gating == 'none'                                         # the gates' own parameters get theirs
    for n in sorted(go):
        big = float(go[n].abs().max())
        assert big > 0 and gn[n].shape == go[n].shape, n
        rel = float((gn[n] - go[n]).abs().max()) / big
        print('  %-40s %.3g' % (n, rel))
        assert rel <= 1e-10, (n, rel)


@pytest.mark.parametrize('T', [1, 6])
@pytest.mark.parametrize('gating', list(GATINGS))
def test_model_fp32_no_further_from_the_fp64_truth(gating, T, spy, monkeypatch):
    m64 = _model(gating, sigma2=torch.nn.Tanh).to(DEV)                             # (a smooth head: no kink for fp32 to fall across)
    m32 = copy.deepcopy(m64).float()
    x, h0, y = _inputs(T)
    lgn, gn = _step(m32, x.float(), h0.float(), y)
    _new_path_only(spy, backward=True)
    monkeypatch.setenv(SWITCH, '1')
    spy.calls.clear()
    lgo, go = _step(m32, x.float(), h0.float(), y)
    _old_path_only(spy)
    lgt, truth = _step(m64, x, h0, y)
    assert set(gn) == set(go) == set(truth)
    eps = torch.finfo(F32).eps
    gn, go, truth = dict(gn, logits=lgn), dict(go, logits=lgo), dict(truth, logits=lgt)
    for n in sorted(truth):
        g = truth[n]
        e_new, e_old = float((gn[n].double() - g).abs().max()), float((go[n].double() - g).abs().max())
        print('%s T=%d %-40s new %.3g two-module %.3g' % (gating, T, n, e_new, e_old))
        assert e_new <= 2 * e_old + 16 * eps * float(g.abs().max()), (n, e_new, e_old)


def _g15(name, dt):
    from test_gnn_heads import _model as g15_model
    g = load_golden(name)
    m = g15_model(name, g).double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    return g, m.to(DEV).to(dt)


def _g15_check(name, g, m, dt, tol):
    x = torch.tensor(g['x'], dtype=dt, device=DEV, requires_grad=True)
    h0 = torch.tensor(g['h0'], dtype=dt, device=DEV, requires_grad=True)
    y = m(x, h0)
    (y * torch.tensor(g['R'], dtype=dt, device=DEV)).sum().backward()

    def close(a, ref, what, tol):
        a = a.detach().double().cpu().numpy()
        assert a.shape == ref.shape, (what, a.shape, ref.shape)
        err = float(np.max(np.abs(a - ref))) / max(1.0, float(np.max(np.abs(ref))))
        print('%s %s %-36s %.3g' % (name, dt, what, err))
        assert err <= tol, '%s %s: rel err %g' % (name, what, err)
    cell_tol = tol if dt == F64 else 1e-4                  # test_gnn_heads.py's tolerances
    close(y, g['y'], 'y', tol)
    seen = 0
    for k, p in m.named_parameters():
        if k in g['grads']:
            close(p.grad, g['grads'][k], k, cell_tol if k.startswith('stateGCRNN.') else tol)
            seen += 1
    assert seen >= 7
    close(x.grad, g['grad_x'], 'x', cell_tol)
    close(h0.grad, g['grad_h0'], 'h0', cell_tol)


@pytest.mark.parametrize('name', ['g15_cls_gcrnngnn_none', 'g15_cls_gcrnngnn_time'])
@pytest.mark.parametrize('dt,tol', [(F64, 1e-11), (F32, 1e-5)])
def test_reference_fixtures_on_the_new_path(dt, tol, name, spy):
    g, m = _g15(name, dt)
    _g15_check(name, g, m, dt, tol)
    _new_path_only(spy, backward=True)


def test_reference_adam_trace_on_the_new_path(spy):
    g = load_golden('g15_trace_gcrnngnn')
    from test_gnn_heads import _model as g15_model
    m = g15_model('g15_cls_gcrnngnn_none', g).double()
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
    _new_path_only(spy, backward=True)
    assert spy.calls[FWD_CLS] == 10 and spy.calls[BWD_CLS] == 10


def test_graphed_train_step_replays_the_eager_step(spy):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import GraphedTrainStep, train_step
    from gated_gcrnns_amd.Utils.miscTools import CrossEntropyLoss
    me = _model('time').to(DEV)
    mg = copy.deepcopy(me)
    x, _, y = _inputs(5, B=4)
    oe = optim.make_trainer('ADAM', me.parameters(), 1e-3, 0.9, 0.999, flat=True)
    og = optim.make_trainer('ADAM', mg.parameters(), 1e-3, 0.9, 0.999, flat=True)
    le, lg = CrossEntropyLoss(), CrossEntropyLoss()
    stepper = GraphedTrainStep(mg, lg, og, x, y, 20)                               # three eager warm-up steps, then the capture
    assert stepper.captured
    assert spy.calls[BWD_CLS] == 4 and spy.calls[FWD_CLS] == 4 and spy.calls[D_BWD] == 0 and spy.calls['small_cell_train'] == 0 \
        and spy.calls['graph_filter_layer'] == 0, dict(spy.calls)
    for _ in range(3):
        train_step(me, le, oe, x, y, 20)
    for it in range(3):
        xb = torch.roll(x, it + 1, dims=0)                                         # fresh inputs every replay
        yb = torch.roll(y, it + 1, dims=0)
        loss_e, yhat_e = train_step(me, le, oe, xb, yb, 20)
        loss_g, yhat_g = stepper(xb, yb)
        assert torch.equal(loss_e, loss_g) and torch.equal(yhat_e, yhat_g), it
        assert all(torch.equal(a, b) for a, b in zip(me.parameters(), mg.parameters())), it
    assert spy.calls[BWD_CLS] == 4 + 6, dict(spy.calls)                            # replays launch without passing through Python


def test_neither_the_states_nor_dh_are_allocated(spy, monkeypatch):
    """Un-gated model, fp64, T = 50, B = 8: one B T F N buffer is 3.78 MB. A training step holds the forward's own states (one such
    buffer) and, with no dH, less than one more above them: the slots, V, dU and the logits are B-sized. The two-module path adds the
    zero-filled dH of `select`, a whole second buffer. Inference stores no state: its peak is below one buffer (the two-module path stores
    the last state alone, so it has no lower bound to assert). The caps follow from these allocation counts; the observed figures are
    printed."""
    B, T, F, N = 8, 50, 20, 59
    states = B * T * F * N * 8
    m = _model('none').to(DEV)
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(B, T, 1, N, generator=gen, dtype=F64).to(DEV)
    h0 = (0.3 * torch.randn(B, F, N, generator=gen, dtype=F64)).to(DEV)
    y = torch.randint(0, 11, (B,), generator=gen).to(DEV)

    def infer():
        with torch.no_grad():
            return m(x, h0)

    def train():
        m.zero_grad(set_to_none=True)
        lg = m(x, h0)
        ops().cross_entropy(lg, y).backward()
        return lg.detach()
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
    assert seen['infer', False] < states
    assert seen['train', False] < 2 * states                                        # the forward's own states and less than one more buffer
    assert seen['train', True] >= 2 * states                                        # H and the dH of select
    for name in ('infer', 'train'):
        assert float((seen[name, False, 'y'] - seen[name, True, 'y']).abs().max()) <= 1e-10 and _spread(seen[name, False, 'y'])


def test_default_dispatch_follows_the_measurement(spy, monkeypatch):
    """Without GCRNN_SMALL_CLS_GNN_HEAD=all the model takes the new path exactly where GGCRNNCell._small_cls_gnn_head_pays says so, on each
    measured row (fp32 / fp64, T = 5 / 20 / 200, inference and training step); =all overrides it; either way the same numbers."""
    import gated_gcrnns_amd.Utils.graphML as gml
    m64 = _model('none').to(DEV)
    models = {F64: m64, F32: copy.deepcopy(m64).float()}
    for dt in (F64, F32):
        m = models[dt]
        for T in (5, 20, 200):
            gen = torch.Generator().manual_seed(T)
            x, h0 = (torch.randn(*s, generator=gen, dtype=F64).to(DEV).to(dt) for s in ((2, T, 1, 59), (2, 20, 59)))
            y = torch.randint(0, 11, (2,), generator=gen).to(DEV)
            for take_all in (False, True):
                if take_all:
                    monkeypatch.setenv(TAKE_ALL, 'all')
                else:
                    monkeypatch.delenv(TAKE_ALL, raising=False)
                spy.calls.clear()
                with torch.no_grad():
                    lg = m(x, h0)
                if take_all or gml.GGCRNNCell._small_cls_gnn_head_pays(x, False):
                    _new_path_only(spy, backward=False)
                else:
                    _old_path_only(spy)
                spy.calls.clear()
                lgs, g = _step(m, x, h0, y)
                if take_all or gml.GGCRNNCell._small_cls_gnn_head_pays(x, True):
                    _new_path_only(spy, backward=True)
                else:
                    _old_path_only(spy)
            monkeypatch.setenv(SWITCH, '1')
            lg2, g2 = _step(m, x, h0, y)
            monkeypatch.delenv(SWITCH)
            tol = 1e-10 if dt == F64 else 1e-3
            assert float((lgs - lg2).abs().max()) <= tol * max(1.0, float(lg2.abs().max())) and set(g) == set(g2)
            assert float((lg - lg2).abs().max()) <= tol * max(1.0, float(lg2.abs().max()))
            for n in g2:
                assert float((g[n] - g2[n]).abs().max()) <= tol * float(g2[n].abs().max()), (dt, T, n)


def test_a_final_nonlinearity_is_applied_to_the_logits(spy, monkeypatch):
    x, h0, _ = _inputs(5)
    sig = _model('none', final=torch.nn.Sigmoid).to(DEV)
    with torch.no_grad():
        p_new = sig(x, h0)
    _new_path_only(spy, backward=False)
    monkeypatch.setenv(SWITCH, '1')
    spy.calls.clear()
    with torch.no_grad():
        p_old = sig(x, h0)
    _old_path_only(spy)
    assert tuple(p_new.shape) == (3, 11) == tuple(p_old.shape) and float(p_new.min()) > 0 and float(p_new.max()) < 1 and _spread(p_new)
    assert float((p_new - p_old).abs().max()) <= 1e-10
