"""Input gradient of the edge-gated cell in the small-graph regime (csrc/gcrnn_small_edge_bwd.hip with DX, gcrnn_small_edge_backward_dx,
ops.small_edge_cell_train with an X that requires grad, GGCRNNCell._use_small_edge_training under GCRNN_SMALL_EDGE_DX=1): the input-branch
launch of the BPTT goes on to the adjoint of the hops and returns dX; no launch is added.

Gradient reference: oracle/torch_reference.py::ggcrnn_cell under CPU fp64 autograd with X as a leaf that requires grad (and the g3
fixtures' grad_*_X). Bounds are the project's standing ones (TOLS of tests/test_fp64_envelopes.py): states max-abs <= 1e-11 (fp64) /
1e-5 (fp32); every gradient, dX included, max-abs error / max|ref| <= 1e-10 / 2e-5. "Path taken" is checked with a call counter on the
library's entry points. The module takes the new path only with GCRNN_SMALL_EDGE_DX=1 (the `spy` fixture sets it).
"""
import collections
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import torch_reference as tr

TOLS = {torch.float64: (1e-11, 1e-10), torch.float32: (1e-5, 2e-5)}
DTYPES = [torch.float64, torch.float32]
DX, BWD, FWD = 'gcrnn_small_edge_backward_dx', 'gcrnn_small_edge_backward', 'gcrnn_small_edge_forward'
COMPOSED = ('gcrnn_attention_forward', 'gcrnn_attention_backward', 'gcrnn_taps_forward')
VAR, OFF = 'GCRNN_SMALL_EDGE_DX', 'GCRNN_NO_SMALL_EDGE'


def gml():
    import gated_gcrnns_amd.Utils.graphML as m
    return m


def ops():
    from gated_gcrnns_amd import ops as m
    return m


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


class _CountingLib(object):
    """ops.lib with a call counter on every compute entry point (the queries pass through)."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('gcrnn_') or name.endswith(('_supported', '_parts', '_slots', '_blocks', '_version')):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def spy(monkeypatch):
    s = _CountingLib(ops().lib)
    monkeypatch.setattr(ops(), 'lib', s)
    monkeypatch.delenv(OFF, raising=False)
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    monkeypatch.setenv(VAR, '1')
    return s


def new_path_only(spy, dx=1, plain=0):
    assert spy.calls[DX] == dx and spy.calls[BWD] == plain and spy.calls[FWD] == dx + plain, dict(spy.calls)
    for name in COMPOSED:
        assert spy.calls[name] == 0, dict(spy.calls)


def Tn(a, dt, dev):
    return torch.tensor(np.asarray(a), dtype=dt, device=dev)


def rel_err(got, ref):
    ref = torch.as_tensor(np.asarray(ref) if not isinstance(ref, torch.Tensor) else ref).double().reshape(-1)
    got = got.detach().double().cpu().reshape(-1)
    assert got.numel() == ref.numel()
    assert bool(torch.isfinite(got).all())
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


# ---------------------------------------------------------------------------------------------- graphs and cases
def gso_adj59():
    return load_golden('g5_cls_T20K4_none')['S']                       # 1 x 59 x 59, the epicenter driver's graph


def gso_sbm50():
    return load_golden('g5_reg_multipMlp_none')['S']                   # 1 x 50 x 50, the SBM of fixture G5


def gso_dir17():
    """Directed, signed weights; S[3][3] = -1 with row 3 otherwise empty (S + I cancels: an empty support row); node 5 isolated
    (its support is the self-loop of S + I alone); row 9 is a hub that reaches every node but the isolated one."""
    rng = np.random.default_rng(17)
    N = 17
    S = (rng.random((N, N)) < 0.2) * rng.uniform(0.2, 1.0, (N, N)) * rng.choice([-1.0, 1.0], (N, N))
    np.fill_diagonal(S, 0.0)
    S[9, :] = rng.uniform(0.2, 1.0, N) * rng.choice([-1.0, 1.0], N)
    S[3, :] = 0.0
    S[3, 3] = -1.0
    S[5, :] = 0.0
    S[:, 5] = 0.0
    S = S / np.abs(S).sum(axis=1).max()
    S[3, 3] = -1.0
    return S.reshape(1, N, N)


def gso_rand80():
    rng = np.random.default_rng(80)
    N = 80
    S = (rng.random((N, N)) < 0.1) * rng.uniform(0.1, 1.0, (N, N))
    np.fill_diagonal(S, 0.0)
    return (S / np.abs(S).sum(axis=1).max()).reshape(1, N, N)


#        name        graph      G  F   Kin Kst T    B  bias
CASES = {'dir17':   (gso_dir17, 3, 7, 3, 2, 3, 2, True),
         'k1':      (gso_dir17, 3, 7, 1, 1, 3, 2, True),              # no hop: dX = dz_0
         'nobias':  (gso_dir17, 3, 7, 3, 2, 3, 2, False),
         'gwide':   (gso_dir17, 9, 4, 2, 4, 3, 2, True),              # G > F: C = G sets the buffer rows; Kin < Kst
         'quake':   (gso_adj59, 1, 20, 4, 4, 20, 3, True),
         'kstep':   (gso_sbm50, 1, 20, 5, 5, 5, 4, True),
         'rand80':  (gso_rand80, 1, 32, 3, 3, 200, 2, True),
         'rand80f20': (gso_rand80, 1, 20, 3, 3, 200, 2, True)}
_REFS = {}


def make_cell(S, G, F, Kin, Kst, tg, bias, seed):
    torch.manual_seed(seed)
    cell = gml().GGCRNNCell(G, F, Kin, Kst, torch.tanh, tg, 'edge', 1, bias)
    cell.addGSO(torch.tensor(S))
    return cell.double()


def reference(cell, S, X, h0, Rw, tg):
    """(H, {parameter name, 'h0' or 'X': gradient}) of loss = (H * Rw).sum() under CPU fp64 autograd, X a leaf."""
    params = {k: v.detach().clone().requires_grad_() for k, v in cell.state_dict().items()}
    Xt, h0t = torch.tensor(X, requires_grad=True), torch.tensor(h0, requires_grad=True)
    H = tr.ggcrnn_cell(params, torch.tensor(S), Xt, h0t, time_gating=tg, spatial_gating='edge')
    (H * torch.tensor(Rw)).sum().backward()
    grads = {k: v.grad.detach() for k, v in params.items() if v.grad is not None}
    grads['h0'], grads['X'] = h0t.grad.detach(), Xt.grad.detach()
    return H.detach(), grads


def case(name, tg):
    """(fp64 cell on the CPU, S, X, h0, R, reference H, reference gradients) -- computed once per (case, gating), never changed."""
    key = (name, tg)
    if key not in _REFS:
        mk, G, F, Kin, Kst, T, B, bias = CASES[name]
        S = mk()
        N = S.shape[1]
        rng = np.random.default_rng(1000 + len(name) + 7 * T)
        cell = make_cell(S, G, F, Kin, Kst, tg, bias, seed=T + N + 1)
        X = rng.standard_normal((B, T, G, N))
        h0 = np.tanh(rng.standard_normal((B, F, N)))
        Rw = rng.standard_normal((B, T, F, N))
        H, grads = reference(cell, S, X, h0, Rw, tg)
        _REFS[key] = (cell, S, X, h0, Rw, H, grads)
    return _REFS[key]


def run_cell(cell, X, h0, Rw, dt, dev, x_grad=True, h_grad=True):
    """One training step of loss = (H * Rw).sum() on the device: (H, {name, 'h0' or 'X': gradient})."""
    cell = copy.deepcopy(cell).to(dev).to(dt)
    Xd, hd = Tn(X, dt, dev).requires_grad_(x_grad), Tn(h0, dt, dev).requires_grad_(h_grad)
    H = cell(Xd, hd)
    (H * Tn(Rw, dt, dev)).sum().backward()
    grads = {k: p.grad for k, p in cell.named_parameters() if p.grad is not None}
    if hd.grad is not None:
        grads['h0'] = hd.grad
    if Xd.grad is not None:
        grads['X'] = Xd.grad
    return H.detach(), grads


def check_all(H, grads, Href, gref, dt, label, expect=None):
    tol_h, tol_g = TOLS[dt]
    err = float((H.double().cpu() - Href).abs().max())
    print('%s %s: states max-abs %.3e' % (label, dt, err))
    assert err <= tol_h
    expect = set(gref) if expect is None else expect
    assert expect <= set(grads), sorted(expect - set(grads))
    for k in sorted(expect):
        e = rel_err(grads[k], gref[k])
        print('%s %s: grad %s rel %.3e' % (label, dt, k, e))
        assert e <= tol_g, k


# ---------------------------------------------------------------------------------------------- 1. reference fixtures
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('loss', ['sum', 'l1'])
@pytest.mark.parametrize('name,tg', [('edge', False), ('time_edge', True)])
def test_reference_fixtures(dev, spy, name, tg, loss, dt):
    g = load_golden('g3_cell_' + name)
    cell = gml().GGCRNNCell(2, 5, 3, 3, torch.tanh, tg, 'edge', 1, True)
    cell.addGSO(torch.tensor(g['S']))
    cell = cell.double()
    cell.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    cell = cell.to(dev).to(dt)
    X, h0 = Tn(g['X'], dt, dev).requires_grad_(), Tn(g['h0'], dt, dev).requires_grad_()
    H = cell(X, h0)
    (H.sum() if loss == 'sum' else torch.nn.L1Loss()(H, Tn(g['target'], dt, dev))).backward()
    gref = dict(g['grad_' + loss])
    gref['h0'], gref['X'] = g['grad_%s_h0' % loss], g['grad_%s_X' % loss]
    grads = {k: p.grad for k, p in cell.named_parameters() if p.grad is not None}
    grads['h0'], grads['X'] = h0.grad, X.grad
    assert {k for k in g['params'] if not k.startswith(('GFL_out', 'MLP_out'))} <= set(gref)      # every parameter the cell uses
    check_all(H.detach(), grads, torch.tensor(g['H']), gref, dt, 'fixture g3_cell_%s %s' % (name, loss))
    new_path_only(spy)


# ---------------------------------------------------------------------------------------------- 2. torch reference
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('name', ['dir17', 'k1', 'nobias', 'gwide', 'quake', 'kstep'])
def test_against_torch_reference(dev, spy, name, tg, dt):
    cell, S, X, h0, Rw, Href, gref = case(name, tg)
    H, grads = run_cell(cell, X, h0, Rw, dt, dev)
    names = {k for k, _ in cell.named_parameters()}
    assert {k for k in names if not k.startswith(('GFL_out', 'MLP_out'))} | {'h0', 'X'} == set(gref)
    assert float(gref['X'].abs().max()) > 0
    check_all(H, grads, Href, gref, dt, 'reference %s time_gating=%s' % (name, tg))
    new_path_only(spy)


# ---------------------------------------------------------------------------------------------- 3. X only
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('tg', [False, True])
def test_only_x_wants_a_gradient(dev, spy, tg, dt):
    """Frozen parameters, h0 without grad (saliency): the new path runs for X alone and no parameter gets a .grad."""
    cell, S, X, h0, Rw, Href, gref = case('dir17', tg)
    frozen = copy.deepcopy(cell)
    for p in frozen.parameters():
        p.requires_grad_(False)
    H, grads = run_cell(frozen, X, h0, Rw, dt, dev, h_grad=False)
    assert set(grads) == {'X'}, sorted(grads)
    check_all(H, grads, Href, gref, dt, 'X only time_gating=%s' % tg, expect={'X'})
    new_path_only(spy)


# ---------------------------------------------------------------------------------------------- 4. ops level
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
def test_ops_level_returns_dx_and_leaves_the_plain_call_alone(dev, spy, monkeypatch, dt):
    """ops.small_edge_cell_train needs no environment: X.requires_grad -> the dx entry once; a detached X -> the plain entry once, and
    the same parameter gradients to the bit."""
    monkeypatch.delenv(VAR)
    cell, S, X, h0, Rw, Href, gref = case('dir17', False)
    cell = copy.deepcopy(cell).to(dev).to(dt)

    def run(x_grad):
        for p in cell.parameters():
            p.grad = None
        Xd, hd = Tn(X, dt, dev).requires_grad_(x_grad), Tn(h0, dt, dev).requires_grad_()
        H = ops().small_edge_cell_train(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph,
                                        (cell.input_attention.mixer, cell.input_attention.weight),
                                        (cell.forget_attention.mixer, cell.forget_attention.weight))
        (H * Tn(Rw, dt, dev)).sum().backward()
        grads = {k: p.grad.clone() for k, p in cell.named_parameters() if p.grad is not None}
        grads['h0'] = hd.grad
        if x_grad:
            grads['X'] = Xd.grad
        else:
            assert Xd.grad is None
        return H.detach(), grads
    H, with_dx = run(True)
    new_path_only(spy, dx=1, plain=0)
    check_all(H, with_dx, Href, gref, dt, 'ops level')
    H2, plain = run(False)
    new_path_only(spy, dx=1, plain=1)
    assert torch.equal(H, H2)
    assert set(plain) == set(with_dx) - {'X'} and len(plain) >= 8
    for k in plain:
        assert torch.equal(plain[k], with_dx[k]), k


# ---------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('tg', [False, True])
def test_determinism_and_batch_independence(dev, spy, tg, dt):
    mk, G, F, Kin, Kst, T, _, bias = CASES['quake']
    S = mk()
    N = S.shape[1]
    cell = make_cell(S, G, F, Kin, Kst, tg, bias, seed=5)
    rng = np.random.default_rng(5)
    X, h0, Rw = rng.standard_normal((5, T, G, N)), np.tanh(rng.standard_normal((5, F, N))), rng.standard_normal((5, T, F, N))
    H1, g1 = run_cell(cell, X, h0, Rw, dt, dev)
    H2, g2 = run_cell(cell, X, h0, Rw, dt, dev)
    assert torch.equal(H1, H2) and set(g1) == set(g2) and len(g1) >= 9 and 'X' in g1
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for b in (0, 3):
        _, gb = run_cell(cell, X[b:b + 1], h0[b:b + 1], Rw[b:b + 1], dt, dev)
        assert torch.equal(gb['X'][0], g1['X'][b]), b
        assert torch.equal(gb['h0'][0], g1['h0'][b]), b
    new_path_only(spy, dx=4)


# ---------------------------------------------------------------------------------------------- 6. stacked cells
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
def test_stacked_cells(dev, spy, dt):
    """Two edge-gated cells, the second fed the first's states, the loss on the second's: the second cell returns dX (the dx entry), the
    first one's X wants nothing (the plain entry); every gradient of both against the same stack in the torch reference."""
    S = gso_dir17()
    N, B, T = 17, 2, 3
    c1, c2 = make_cell(S, 3, 7, 2, 2, False, True, seed=61), make_cell(S, 7, 5, 2, 2, False, True, seed=62)
    rng = np.random.default_rng(6)
    X, Rw = rng.standard_normal((B, T, 3, N)), rng.standard_normal((B, T, 5, N))
    h1, h2 = np.tanh(rng.standard_normal((B, 7, N))), np.tanh(rng.standard_normal((B, 5, N)))
    p1 = {k: v.detach().clone().requires_grad_() for k, v in c1.state_dict().items()}
    p2 = {k: v.detach().clone().requires_grad_() for k, v in c2.state_dict().items()}
    h1t, h2t, St = torch.tensor(h1, requires_grad=True), torch.tensor(h2, requires_grad=True), torch.tensor(S)
    Hmid = tr.ggcrnn_cell(p1, St, torch.tensor(X), h1t, spatial_gating='edge')
    Href = tr.ggcrnn_cell(p2, St, Hmid, h2t, spatial_gating='edge')
    (Href * torch.tensor(Rw)).sum().backward()
    gref = {'1.' + k: v.grad for k, v in p1.items()}
    gref.update({'2.' + k: v.grad for k, v in p2.items()})
    gref['1.h0'], gref['2.h0'] = h1t.grad, h2t.grad
    assert all(v is not None and float(v.abs().max()) > 0 for v in gref.values())
    d1, d2 = copy.deepcopy(c1).to(dev).to(dt), copy.deepcopy(c2).to(dev).to(dt)
    h1d, h2d = Tn(h1, dt, dev).requires_grad_(), Tn(h2, dt, dev).requires_grad_()
    H = d2(d1(Tn(X, dt, dev), h1d), h2d)
    (H * Tn(Rw, dt, dev)).sum().backward()
    grads = {'1.' + k: p.grad for k, p in d1.named_parameters()}
    grads.update({'2.' + k: p.grad for k, p in d2.named_parameters()})
    grads['1.h0'], grads['2.h0'] = h1d.grad, h2d.grad
    check_all(H.detach(), grads, Href.detach(), gref, dt, 'stacked')
    new_path_only(spy, dx=1, plain=1)


# ---------------------------------------------------------------------------------------------- 7. long sequence
@pytest.mark.gpu
def test_long_sequence_fp64(dev, spy):
    """T = 200 in fp64 at the standing bounds on the BPTT kernels themselves (rand80 at F = 20, which fits their LDS)."""
    cell, S, X, h0, Rw, Href, gref = case('rand80f20', False)
    H, grads = run_cell(cell, X, h0, Rw, torch.float64, dev)
    new_path_only(spy)
    check_all(H, grads, Href, gref, torch.float64, 'rand80f20 T=200')


@pytest.mark.gpu
def test_long_sequence_fp32_against_composed_error(dev, spy, monkeypatch):
    """Over 200 steps no fp32 bound can be derived: the composed fp32 path's error against the same fp64 reference is the yardstick, and
    the new path may have max(2e-5, twice that) of each gradient's max (2: another, equally valid, order of summation)."""
    dt = torch.float32
    cell, S, X, h0, Rw, Href, gref = case('rand80', False)
    H, grads = run_cell(cell, X, h0, Rw, dt, dev)
    new_path_only(spy)
    monkeypatch.delenv(VAR)
    Hc, gcomp = run_cell(cell, X, h0, Rw, dt, dev)
    assert spy.calls[DX] == 1 and spy.calls[BWD] == 0 and spy.calls['gcrnn_attention_backward'] > 0, dict(spy.calls)
    e_new, e_old = float((H.double().cpu() - Href).abs().max()), float((Hc.double().cpu() - Href).abs().max())
    print('rand80 fp32 states: new %.3e composed %.3e' % (e_new, e_old))
    assert e_new <= max(1e-5, 2 * e_old)
    assert 'X' in grads and set(gref) <= set(grads) and set(gref) <= set(gcomp)
    for k in sorted(gref):
        e_new, e_old = rel_err(grads[k], gref[k]), rel_err(gcomp[k], gref[k])
        print('rand80 fp32 grad %s: new %.3e composed %.3e' % (k, e_new, e_old))
        assert e_new <= max(2e-5, 2 * e_old), k


# ---------------------------------------------------------------------------------------------- 8. switch
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
def test_no_small_edge_still_wins(dev, spy, monkeypatch, dt):
    monkeypatch.setenv(OFF, '1')
    cell, S, X, h0, Rw, Href, gref = case('dir17', False)
    H, grads = run_cell(cell, X, h0, Rw, dt, dev)
    check_all(H, grads, Href, gref, dt, 'switch')
    assert not [n for n in spy.calls if n.startswith('gcrnn_small_edge')], dict(spy.calls)
    assert spy.calls['gcrnn_attention_backward'] > 0
