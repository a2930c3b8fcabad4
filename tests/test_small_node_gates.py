"""GPU (-m gpu): the node gates of the small-graph regime in one launch forward, one backward (gcrnn_small_node_gates_*,
ops.small_node_gates, GGCRNNCell._small_gates) against the plain-torch fp64 reference (oracle/torch_reference.py: lsigf, graph_filter,
ggcrnn_cell, autograd) and the reference's own fixtures.

Tolerances are the project's (TOLS of test_fp64_envelopes.py): fp64 values <= 1e-11, gradients <= 1e-10 of their own
maximum; fp32 values <= 1e-5, gradients <= 2e-5. Graphs, initialisation and the counting wrapper follow test_small_input_grad.py: directed,
weighted, an isolated node, a hub and self-loops; h0 is non-zero everywhere."""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import torch_reference as tr

pytestmark = pytest.mark.gpu

NG_FWD, NG_BWD, NG_DX = 'gcrnn_small_node_gates_forward', 'gcrnn_small_node_gates_backward', 'gcrnn_small_node_gates_backward_dx'
GT_FWD, GT_BWD, GT_DX = 'gcrnn_small_gates_forward', 'gcrnn_small_gates_backward', 'gcrnn_small_gates_backward_dx'
D_FWD, D_BWD, D_DX = 'gcrnn_small_dense_forward', 'gcrnn_small_dense_backward', 'gcrnn_small_dense_backward_dx'
TOLS = {torch.float64: (1e-11, 1e-10), torch.float32: (1e-5, 2e-5)}
DTS = (torch.float64, torch.float32)
OFF = 'GCRNN_NO_SMALL_NODE_GATES'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


def gml():
    import gated_gcrnns_amd.Utils.graphML as m
    return m


def ops():
    from gated_gcrnns_amd import ops as m
    return m


def archit():
    import gated_gcrnns_amd.Modules.architectures as m
    return m


class _CountingLib(object):
    """ops.lib with a call counter on every compute entry point (queries pass through)."""

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
    return s


@pytest.fixture(autouse=True)
def _matrix_core_family(monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    monkeypatch.delenv(OFF, raising=False)
    monkeypatch.delenv('GCRNN_SMALL_NODE_GATES', raising=False)


@functools.lru_cache(maxsize=None)
def graph(N, seed):
    """1 x N x N GSO, spectral radius 1. Directed, weights in +-[0.2, 1]; node 0 isolated, node 1 a hub with >= N/4 out- and
    in-neighbours, self-loops on N/8 nodes (the generator of test_small_input_grad.py)."""
    rng = np.random.default_rng(seed)
    M = (rng.random((N, N)) < min(1.0, 4.0 / N)).astype(np.float64)
    np.fill_diagonal(M, 0.0)
    if N >= 8:
        nb = rng.choice(np.arange(2, N), size=(N + 3) // 4, replace=False)
        M[1, nb] = 1.0
        M[nb, 1] = 1.0
        loops = rng.choice(np.arange(1, N), size=N // 8, replace=False)
        M[loops, loops] = 1.0
        M[0, :] = 0.0
        M[:, 0] = 0.0
    else:
        M[0, 0] = 1.0
    M *= rng.uniform(0.2, 1.0, (N, N)) * rng.choice([-1.0, 1.0], (N, N), p=[0.3, 0.7])
    M /= np.max(np.abs(np.linalg.eigvals(M)))
    S = M[None]
    if N >= 8:
        assert not np.allclose(S, S.transpose(0, 2, 1)) and np.count_nonzero(S[0, 1]) >= N / 4 and np.count_nonzero(S[0, :, 1]) >= N / 4
    return S


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _close(got, ref, tol, what):
    err = _rel(got, ref)
    print('%s: %.3g' % (what, err))
    assert err <= tol, '%s: %.3g of its maximum' % (what, err)


def _abs_close(got, ref, tol, what):
    err = float((got.double() - ref).abs().max())
    print('%s: %.3g' % (what, err))
    assert err <= tol, '%s: %.3g' % (what, err)


# ---------------------------------------------------------------------------------------------------------------- 1. kernel against the oracle
NAMES = ('wA2', 'wB2', 'bias2', 'wf2', 'bf2')


def gate_inputs(N, G, F, Ki, Ks, B, T, cell_bias=True, filt_bias=True, seed=5):
    """fp64 CPU tensors: X, h0, the stacked parameters (taps at 1/sqrt(fan-in); the filters scaled up so that the gates are far from 0.5), R."""
    gen = torch.Generator().manual_seed(seed + N + 3 * F)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1      # noqa: E731
    p = {'wA2': rnd(2, F, Ki, G) / np.sqrt(G * Ki), 'wB2': rnd(2, F, Ks, F) / np.sqrt(F * Ks),
         'bias2': 0.5 * rnd(2, F) if cell_bias else None,
         'wf2': 3.0 * rnd(2, Ks, F) / np.sqrt(F * Ks), 'bf2': rnd(2) if filt_bias else None}
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64)
    h0 = 0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64) + 0.1
    R = torch.randn(2, B, T, N, generator=gen, dtype=torch.float64)
    return X, h0, p, R


def oracle_gates(X, h0, p, S):
    """[2][B][T][N] from oracle.lsigf / graph_filter: sigmoid(GraphFilter_{F->1}(tanh(A_g(S) x_t + b_g + B_g(S) h0 + b_g)))."""
    F, Ks = p['wf2'].shape[2], p['wf2'].shape[1]
    out = []
    for g in range(2):
        b = p['bias2'][g].reshape(F, 1) if p['bias2'] is not None else None
        bf = p['bf2'][g].reshape(1, 1) if p['bf2'] is not None else None
        yb = tr.lsigf(p['wB2'][g].unsqueeze(1), S, h0, b)
        steps = []
        for t in range(X.shape[1]):
            d = torch.tanh(tr.lsigf(p['wA2'][g].unsqueeze(1), S, X[:, t], b) + yb)
            steps.append(torch.sigmoid(tr.graph_filter(p['wf2'][g].reshape(1, 1, Ks, F), bf, S, d))[:, 0])
        out.append(torch.stack(steps, dim=1))
    return torch.stack(out, dim=0)


def run_gates(dev, spy, N, G, F, Ki, Ks, B, T, cell_bias=True, filt_bias=True, x_grad=True, h0_grad=True, dts=DTS):
    from gated_gcrnns_amd.graph import GraphOperator
    S = graph(N, 1000 + N + 7 * F)
    gop = GraphOperator(S, device=dev)
    X, h0, p, R = gate_inputs(N, G, F, Ki, Ks, B, T, cell_bias, filt_bias)
    Sd = torch.tensor(S, device=dev)
    Xr, h0r = X.to(dev).requires_grad_(True), h0.to(dev).requires_grad_(True)
    pr = {k: (v.to(dev).requires_grad_(True) if v is not None else None) for k, v in p.items()}
    ref = oracle_gates(Xr, h0r, pr, Sd)
    (ref * R.to(dev)).sum().backward()
    out = {}
    for dt in dts:
        vtol, gtol = TOLS[dt]
        for backward in (False, True):
            assert ops().small_node_gates_supported(N, G, F, Ki, Ks, dt, backward=backward), (dt, backward)
        Xd, h0d = X.to(dev).to(dt).requires_grad_(x_grad), h0.to(dev).to(dt).requires_grad_(h0_grad)
        pd = {k: (v.to(dev).to(dt).requires_grad_(True) if v is not None else None) for k, v in p.items()}
        spy.calls.clear()
        gates = ops().small_node_gates(Xd, h0d, pd['wA2'], pd['wB2'], pd['bias2'], pd['wf2'], pd['bf2'], gop)
        assert gates.dtype == dt and tuple(gates.shape) == (2, B, T, N)
        (gates * R.to(dev).to(dt)).sum().backward()
        torch.cuda.synchronize()
        want = NG_DX if x_grad else NG_BWD
        assert spy.calls[NG_FWD] == 1 and spy.calls[want] == 1 and spy.calls[NG_BWD if x_grad else NG_DX] == 0, dict(spy.calls)
        assert not [n for n in spy.calls if n.startswith('gcrnn_taps_')], dict(spy.calls)
        _abs_close(gates.detach(), ref.detach(), vtol, '%s gates' % dt)
        for k in NAMES:
            if p[k] is None:
                continue
            assert pd[k].grad is not None and pd[k].grad.shape == pr[k].grad.shape, k
            _close(pd[k].grad, pr[k].grad, gtol, '%s grad %s' % (dt, k))
        if x_grad:
            _close(Xd.grad, Xr.grad, gtol, '%s grad X' % dt)
        else:
            assert Xd.grad is None
        if h0_grad:
            _close(h0d.grad, h0r.grad, gtol, '%s grad h0' % dt)
        else:
            assert h0d.grad is None
        out[dt] = (gates.detach().clone(), [pd[k].grad.clone() for k in NAMES if p[k] is not None],
                   Xd.grad.clone() if x_grad else None, h0d.grad.clone() if h0_grad else None)
    return out


def shape(cid, N, G, F, Ki, Ks, B, T, **kw):
    return pytest.param(dict(N=N, G=G, F=F, Ki=Ki, Ks=Ks, B=B, T=T, **kw), id=cid)


# N in {1, 15, 16, 17, 33, 59}, G in {1, 3, 17}, F in {1, 5, 17, 20}, (Kin, Kst) in {(1, 1), (1, 3), (3, 1), (2, 5), (5, 2), (8, 8)},
# B in {1, 3}, T in {1, 4}; Kst = 8 with F = 1 is the case whose u_k rows do not fit the state buffers (Kst > F rounded up to 4)
KERNEL = [
    shape('N1', 1, 1, 1, 1, 1, 1, 1),
    shape('N15-G3-F5-K1,3', 15, 3, 5, 1, 3, 3, 4),
    shape('N16-G1-F17-K3,1', 16, 1, 17, 3, 1, 1, 4),
    shape('N17-G17-F1-K8,8-rows-outside', 17, 17, 1, 8, 8, 3, 1),
    shape('N33-G3-F20-K2,5', 33, 3, 20, 2, 5, 3, 4),
    shape('N59-G1-F20-K5,2', 59, 1, 20, 5, 2, 3, 4),
    shape('N59-G3-F17-K8,8', 59, 3, 17, 8, 8, 1, 4),
    shape('N33-G17-F5-K1,1', 33, 17, 5, 1, 1, 3, 1),
    shape('no-cell-bias', 33, 3, 5, 2, 5, 3, 4, cell_bias=False),
    shape('no-filter-bias', 17, 1, 20, 5, 2, 3, 4, filt_bias=False),
    shape('no-bias-at-all', 15, 3, 17, 3, 1, 1, 4, cell_bias=False, filt_bias=False),
    shape('X-without-grad', 33, 3, 5, 2, 5, 3, 4, x_grad=False),
    shape('h0-without-grad', 33, 3, 5, 2, 5, 3, 4, h0_grad=False),
    shape('neither-X-nor-h0', 17, 1, 20, 1, 3, 3, 4, x_grad=False, h0_grad=False),
]


@pytest.mark.parametrize('c', KERNEL)
def test_kernel_against_the_oracle(c, dev, spy):
    run_gates(dev, spy, **c)


def test_kernel_long_sequence(dev, spy):
    """T = 200 (N = 20, B = 2): the per-sequence sums over 200 steps. Both dtypes: on this same input the switched-off (composed) fp32 path
    stays inside 2e-5 (gates 1.2e-7, gradients 1.0e-7 .. 1.6e-6 of their maximum; the one-launch path 1.5e-7 and 1.8e-7 .. 2.3e-6), so
    fp32 is held to the tolerance here as well."""
    run_gates(dev, spy, 20, 1, 5, 3, 3, 2, 200)


# ---------------------------------------------------------------------------------------------------------------- 2. which code ran
def _init(cell, G, F, Ki, Ks):
    with torch.no_grad():
        for name, p in cell.named_parameters():
            if name.endswith('weight_A'):
                p.uniform_(-1.0, 1.0).mul_(1.0 / np.sqrt(G * Ki))
            elif name.endswith('weight_B'):
                p.uniform_(-1.0, 1.0).mul_(1.0 / np.sqrt(F * Ks))
            elif name.startswith('MLP_'):
                p.mul_(6.0)
            elif name.startswith('GFL_node_'):
                p.mul_(3.0)
    ops().parameters_changed()


def make_cell(N, G, F, Ki, Ks, tg):
    S = graph(N, 1000 + N + 7 * F)
    torch.manual_seed(N + F)
    cell = gml().GGCRNNCell(G, F, Ki, Ks, torch.tanh, tg, 'node', 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.double()
    _init(cell, G, F, Ki, Ks)
    return cell, S


def _taps_ran(spy):
    return [n for n in spy.calls if n.startswith('gcrnn_taps_')]


CELL = dict(N=33, G=2, F=8, Ki=3, Ks=2, B=3, T=4)


@pytest.mark.parametrize('mode', ['inference', 'training', 'training-dx'])
@pytest.mark.parametrize('tg', [False, True], ids=['node', 'time+node'])
def test_cell_runs_the_new_entry_points(dev, spy, monkeypatch, tg, mode):
    N, G, F, Ki, Ks, B, T = (CELL[k] for k in ('N', 'G', 'F', 'Ki', 'Ks', 'B', 'T'))
    cell, S = make_cell(N, G, F, Ki, Ks, tg)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64).to(dev)
    h0 = (0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64) + 0.1).to(dev)
    R = torch.randn(B, T, F, N, generator=gen, dtype=torch.float64).to(dev)
    Sd = torch.tensor(S, device=dev)
    train, x_grad = mode != 'inference', mode == 'training-dx'
    rp = {k: v.detach().to(dev).clone().requires_grad_(train) for k, v in cell.state_dict().items()}
    Xr, h0r = X.clone().requires_grad_(x_grad), h0.clone().requires_grad_(train)
    Hr = tr.ggcrnn_cell(rp, Sd, Xr, h0r, tg, 'node')
    if train:
        (Hr * R).sum().backward()
    for dt in DTS:
        stol, gtol = TOLS[dt]
        res = {}
        for off in (False, True):
            if off:
                monkeypatch.setenv(OFF, '1')
            else:
                monkeypatch.delenv(OFF, raising=False)
            cd = copy.deepcopy(cell).to(dev).to(dt)
            for p in cd.parameters():
                p.requires_grad_(train)
            Xd, h0d = X.to(dt).clone().requires_grad_(x_grad), h0.to(dt).clone().requires_grad_(train)
            spy.calls.clear()
            if train:
                H = cd(Xd, h0d)
                (H * R.to(dt)).sum().backward()
            else:
                with torch.no_grad():
                    H = cd(Xd, h0d)
            torch.cuda.synchronize()
            what = '%s %s off=%s: %s' % (dt, mode, off, dict(spy.calls))
            assert spy.calls[D_FWD] == 1, what
            if train:
                assert spy.calls[D_DX if x_grad else D_BWD] == 1, what
            if off:
                assert _taps_ran(spy) and not spy.calls[NG_FWD] and not spy.calls[NG_BWD] and not spy.calls[NG_DX], what
            else:
                assert not _taps_ran(spy) and spy.calls[NG_FWD] == 1, what
                assert spy.calls[NG_DX] == (1 if x_grad else 0) and spy.calls[NG_BWD] == (1 if train and not x_grad else 0), what
                assert spy.calls[GT_FWD] == (1 if tg else 0), what
            grads = {k: p.grad for k, p in cd.named_parameters()}
            grads['X'], grads['h0'] = Xd.grad, h0d.grad
            res[off] = (H.detach(), grads)
            _abs_close(H.detach(), Hr.detach(), stol, '%s off=%s states' % (dt, off))
            if train:
                for k, v in rp.items():
                    if v.grad is None or float(v.grad.abs().max()) == 0.0:
                        assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
                        continue
                    _close(grads[k], v.grad, gtol, '%s off=%s grad %s' % (dt, off, k))
                _close(h0d.grad, h0r.grad, gtol, '%s off=%s grad h0' % (dt, off))
                if x_grad:
                    _close(Xd.grad, Xr.grad, gtol, '%s off=%s grad X' % (dt, off))
        # the two paths against each other
        _abs_close(res[False][0], res[True][0].double(), stol, '%s states, new against composed' % dt)
        for k, gnew in res[False][1].items():
            gold = res[True][1][k]
            if gold is None or float(gold.abs().max()) == 0.0:
                assert gnew is None or float(gnew.abs().max()) == 0.0, k
                continue
            _close(gnew, gold.double(), gtol, '%s grad %s, new against composed' % (dt, k))


def test_rows_kept_off_the_dispatch(dev, spy, monkeypatch):
    """GGCRNNCell._small_node_gates_pays: the bare cell's fp32 inference beyond T = 20 keeps the composed pass unless
    GCRNN_SMALL_NODE_GATES=all; T = 20, fp64 and the training step take the new gates."""
    N, G, F, Ki, Ks, B = 17, 1, 5, 2, 2, 2
    cell, _ = make_cell(N, G, F, Ki, Ks, False)
    cell = cell.to(dev)
    for dt, T, every, new in ((torch.float32, 21, False, False), (torch.float32, 21, True, True), (torch.float32, 20, False, True),
                              (torch.float64, 21, False, True)):
        if every:
            monkeypatch.setenv('GCRNN_SMALL_NODE_GATES', 'all')
        else:
            monkeypatch.delenv('GCRNN_SMALL_NODE_GATES', raising=False)
        cd = copy.deepcopy(cell).to(dt)
        X, h0 = torch.randn(B, T, G, N, dtype=dt, device=dev), torch.zeros(B, F, N, dtype=dt, device=dev)
        spy.calls.clear()
        with torch.no_grad():
            cd(X, h0)
        assert spy.calls[NG_FWD] == (1 if new else 0) and bool(_taps_ran(spy)) == (not new), (dt, T, every, dict(spy.calls))
        assert spy.calls[D_FWD] == 1
    monkeypatch.delenv('GCRNN_SMALL_NODE_GATES', raising=False)
    cd = copy.deepcopy(cell).to(torch.float32)
    X, h0 = torch.randn(B, 21, G, N, dtype=torch.float32, device=dev), torch.zeros(B, F, N, dtype=torch.float32, device=dev)
    spy.calls.clear()
    cd(X, h0).sum().backward()
    assert spy.calls[NG_FWD] == 1 and spy.calls[NG_BWD] == 1 and not _taps_ran(spy), dict(spy.calls)


def _model(kind, S, dev, dt):
    torch.manual_seed(3)
    if kind == 'regression':
        m = archit().GatedGCRNNforRegression(1, 8, 3, 3, torch.tanh, torch.nn.ReLU, [1], S[0], True, time_gating=False,
                                             spatial_gating='node', mlpType='multipMlp')
    else:
        m = archit().GatedGCRNNforClassification(1, 8, 3, 3, torch.tanh, torch.nn.ReLU, [5], S[0], True, time_gating=True,
                                                 spatial_gating='node')
    return m.to(dev).to(dt)


@pytest.mark.parametrize('dt', DTS, ids=['fp64', 'fp32'])
@pytest.mark.parametrize('kind', ['regression', 'classification'])
def test_models_reach_the_new_gates_through_their_heads(dev, spy, monkeypatch, kind, dt):
    N, B, T = 33, 3, 4
    S = graph(N, 1000 + N + 7 * 8)
    stol, gtol = TOLS[dt]
    gen = torch.Generator().manual_seed(9)
    X = torch.randn(B, T, 1, N, generator=gen, dtype=torch.float64).to(dev).to(dt)
    h0 = (0.5 * torch.randn(B, 8, N, generator=gen, dtype=torch.float64) + 0.1).to(dev).to(dt)
    base = _model(kind, S, dev, torch.float64)
    res = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv(OFF, '1')
        else:
            monkeypatch.delenv(OFF, raising=False)
        m = copy.deepcopy(base).to(dt)
        ops().parameters_changed()
        spy.calls.clear()
        with torch.no_grad():
            y_inf = m(X, h0)
        torch.cuda.synchronize()
        what = '%s inference off=%s: %s' % (kind, off, dict(spy.calls))
        if off:
            assert _taps_ran(spy) and not spy.calls[NG_FWD], what
        else:
            assert not _taps_ran(spy) and spy.calls[NG_FWD] == 1, what
        spy.calls.clear()
        y = m(X, h0)
        y.square().sum().backward()
        torch.cuda.synchronize()
        what = '%s training off=%s: %s' % (kind, off, dict(spy.calls))
        if off:
            assert _taps_ran(spy) and not spy.calls[NG_FWD] and not spy.calls[NG_BWD] and not spy.calls[NG_DX], what
        else:
            assert not _taps_ran(spy) and spy.calls[NG_FWD] == 1 and spy.calls[NG_BWD] == 1 and spy.calls[NG_DX] == 0, what
        res[off] = (y_inf, y.detach(), {k: p.grad for k, p in m.named_parameters()})
    # values: absolute; the outputs here are O(1)
    _abs_close(res[False][0], res[True][0].double(), stol, 'inference output')
    _abs_close(res[False][1], res[True][1].double(), stol, 'training output')
    for k, gnew in res[False][2].items():
        gold = res[True][2][k]
        if gold is None or float(gold.abs().max()) == 0.0:
            assert gnew is None or float(gnew.abs().max()) == 0.0, k
            continue
        _close(gnew, gold.double(), gtol, 'grad %s' % k)


# ---------------------------------------------------------------------------------------------------------------- 3. reference fixtures
def _relnp(t, ref):
    return float(np.max(np.abs(t.detach().double().cpu().numpy() - ref)) / (np.max(np.abs(ref)) + 1e-30))


@pytest.mark.parametrize('dt', DTS, ids=['fp64', 'fp32'])
@pytest.mark.parametrize('name,tg', [('node', False), ('time_node', True)])
def test_reference_fixtures(dev, spy, name, tg, dt):
    """g3_cell_node / g3_cell_time_node (N = 30, G = 2, F = 5, K = 3, B = 3, T = 4): the states and the gradients of both losses the
    fixtures store, through the new gates (counted)."""
    g = load_golden('g3_cell_' + name)
    stol, gtol = TOLS[dt]
    cell = gml().GGCRNNCell(2, 5, 3, 3, torch.tanh, tg, 'node', 1, True)
    cell.addGSO(torch.tensor(g['S']))
    cell = cell.double()
    cell.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    cell = cell.to(dev).to(dt)
    ops().parameters_changed()
    X = torch.tensor(g['X'], dtype=dt, device=dev, requires_grad=True)
    h0 = torch.tensor(g['h0'], dtype=dt, device=dev, requires_grad=True)

    def counted(what):
        assert spy.calls[NG_FWD] == 1 and spy.calls[NG_DX] == 1 and spy.calls[NG_BWD] == 0 and not _taps_ran(spy), (what, dict(spy.calls))
        assert spy.calls[D_FWD] == 1 and spy.calls[D_DX] == 1, (what, dict(spy.calls))

    spy.calls.clear()
    H = cell(X, h0)
    assert float(np.max(np.abs(H.detach().double().cpu().numpy() - g['H']))) <= stol
    H.sum().backward()
    torch.cuda.synchronize()
    counted('sum loss')
    for k, p in cell.named_parameters():
        ref = g['grad_sum'].get(k)
        if ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            assert _relnp(p.grad, ref) <= gtol, k
    assert _relnp(X.grad, g['grad_sum_X']) <= gtol
    assert _relnp(h0.grad, g['grad_sum_h0']) <= gtol
    cell.zero_grad()
    X.grad = None
    h0.grad = None
    spy.calls.clear()
    torch.nn.L1Loss()(cell(X, h0), torch.tensor(g['target'], dtype=dt, device=dev)).backward()
    torch.cuda.synchronize()
    counted('L1 loss')
    for k, p in cell.named_parameters():
        ref = g['grad_l1'].get(k)
        if ref is not None:
            assert _relnp(p.grad, ref) <= gtol, k
    assert _relnp(X.grad, g['grad_l1_X']) <= gtol


# ---------------------------------------------------------------------------------------------------------------- 4. bit reproducibility
def test_two_runs_give_the_same_bits(dev, spy):
    a = run_gates(dev, spy, 33, 3, 20, 2, 5, 3, 4)
    b = run_gates(dev, spy, 33, 3, 20, 2, 5, 3, 4)
    for dt in DTS:
        ga, pa, xa, ha = a[dt]
        gb, pb, xb, hb = b[dt]
        assert torch.equal(ga, gb) and torch.equal(xa, xb) and torch.equal(ha, hb), dt
        for u, v in zip(pa, pb):
            assert torch.equal(u, v), dt


# ---------------------------------------------------------------------------------------------------------------- 5. every output written
@pytest.mark.parametrize('dt', DTS, ids=['fp64', 'fp32'])
@pytest.mark.parametrize('Ks', [2, 8], ids=['rows-in-state-buffers', 'rows-outside'])
def test_every_output_element_is_written(dev, dt, Ks):
    """The entry points on NaN-prefilled outputs and partial buffers: N = 17 is no multiple of 4, F = 5 none of 16 (nor of 4)."""
    from gated_gcrnns_amd.graph import GraphOperator
    o = ops()
    N, G, F, Ki, B, T = 17, 3, 5, 3, 3, 4
    S = graph(N, 1000 + N + 7 * F)
    Sd = GraphOperator(S, device=dev).dense(dt)
    X, h0, p, R = gate_inputs(N, G, F, Ki, Ks, B, T)
    X, h0, R = X.to(dev).to(dt), h0.to(dev).to(dt), R.to(dev).to(dt)
    p = {k: v.to(dev).to(dt).contiguous() for k, v in p.items()}
    nan = lambda *s: torch.full(s, float('nan'), dtype=dt, device=dev)      # noqa: E731
    P, code, dims = o._p, o.dtype_code(dt), (B, T, N, G, F, Ki, Ks)
    gate = nan(2, B, T, N)
    o.check(o.lib.gcrnn_small_node_gates_forward(code, P(X), P(h0), P(p['wA2']), P(p['wB2']), P(p['bias2']), P(p['wf2']), P(p['bf2']), P(Sd),
                                                 P(gate), *dims, o._stream()), 'fwd')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gate).all())
    dl = (R * gate * (1 - gate)).contiguous()
    for dx in (False, True):
        outs = [nan(B, 2, F, Ki, G), nan(B, 2, F, Ks, F), nan(B, 2, F), nan(B, 2, Ks, F), nan(B, 2), nan(B, 2, F, N)]
        if dx:
            outs.append(nan(B, 2, T, G, N))
        fn = o.lib.gcrnn_small_node_gates_backward_dx if dx else o.lib.gcrnn_small_node_gates_backward
        o.check(fn(code, P(X), P(h0), P(p['wA2']), P(p['wB2']), P(p['bias2']), P(p['wf2']), P(Sd), P(dl), *[P(t) for t in outs], *dims,
                   o._stream()), 'bwd')
        torch.cuda.synchronize()
        for i, t in enumerate(outs):
            assert bool(torch.isfinite(t).all()), (dx, i)


# ---------------------------------------------------------------------------------------------------------------- 6. containment
@pytest.mark.parametrize('dt', DTS, ids=['fp64', 'fp32'])
def test_non_finite_input_stays_in_its_sequence_and_step(dev, spy, dt):
    """The gates read (x_t, h0) only: a NaN x_t (every channel and node of X[b0, t0]) makes gate[:, b0, t0, :] non-finite and nothing else;
    an Inf in h0[b0] touches sequence b0 only, and what it leaves of sequence b0 is no NaN in the other sequences."""
    from gated_gcrnns_amd.graph import GraphOperator
    N, G, F, Ki, Ks, B, T = 33, 3, 5, 2, 5, 3, 4
    S = graph(N, 1000 + N + 7 * F)
    gop = GraphOperator(S, device=dev)
    X, h0, p, _ = gate_inputs(N, G, F, Ki, Ks, B, T)
    X, h0 = X.to(dev).to(dt), h0.to(dev).to(dt)
    p = {k: v.to(dev).to(dt) for k, v in p.items()}
    run = lambda x, h: ops().small_node_gates(x, h, p['wA2'], p['wB2'], p['bias2'], p['wf2'], p['bf2'], gop)      # noqa: E731
    with torch.no_grad():
        clean = run(X, h0)
        b0, t0 = 1, 2
        Xn = X.clone()
        Xn[b0, t0] = float('nan')
        got = run(Xn, h0)
        bad = ~torch.isfinite(got)
        want = torch.zeros_like(bad)
        want[:, b0, t0, :] = True
        assert torch.equal(bad, want)
        assert torch.equal(got[~want], clean[~want])
        hn = h0.clone()
        hn[b0, 2, 5] = float('inf')
        got = run(X, hn)
        keep = torch.ones(B, dtype=torch.bool, device=dev)
        keep[b0] = False
        assert torch.equal(got[:, keep], clean[:, keep])


# ---------------------------------------------------------------------------------------------------------------- 7. saturation
@pytest.mark.parametrize('bf', [40.0, -40.0, -120.0], ids=['bias+40', 'bias-40', 'bias-120'])
def test_saturated_gates_fp32(dev, spy, bf):
    """A saturating filter bias in fp32. +40: the gates are exactly 1 (1 + e^-40 rounds to 1) and every gradient through them is exactly
    zero. -120: e^120 overflows, the gates are exactly 0 and every gradient exactly zero. -40: fp32 does not round sigmoid(-40) = 4.2e-18
    to zero (torch.sigmoid does not either), so there the gates are held to that value (<= 1e-17, and > 0) and the gradients to finite
    and <= 1e-14 in absolute value: e^-40 times sums of at most a few hundred O(1) terms."""
    from gated_gcrnns_amd.graph import GraphOperator
    dt = torch.float32
    sign = 1.0 if bf > 0 else -1.0
    N, G, F, Ki, Ks, B, T = 17, 3, 5, 2, 5, 3, 4
    S = graph(N, 1000 + N + 7 * F)
    gop = GraphOperator(S, device=dev)
    X, h0, p, R = gate_inputs(N, G, F, Ki, Ks, B, T)
    p['wf2'] = p['wf2'] / 300.0                   # the filter moves the pre-sigmoid value by < 0.05: the bias decides
    p['bf2'] = torch.full((2,), bf, dtype=torch.float64)
    Xd, h0d = X.to(dev).to(dt).requires_grad_(True), h0.to(dev).to(dt).requires_grad_(True)
    pd = {k: v.to(dev).to(dt).requires_grad_(True) for k, v in p.items()}
    gates = ops().small_node_gates(Xd, h0d, pd['wA2'], pd['wB2'], pd['bias2'], pd['wf2'], pd['bf2'], gop)
    exact = bf != -40.0
    if exact:
        assert torch.equal(gates.detach(), torch.full_like(gates, 1.0 if sign > 0 else 0.0))
    else:
        assert float(gates.min()) > 0.0 and float(gates.max()) <= 1e-17
    (gates * R.to(dev).to(dt)).sum().backward()
    torch.cuda.synchronize()
    for k, t in list(pd.items()) + [('X', Xd), ('h0', h0d)]:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()), k
        assert float(t.grad.abs().max()) <= (0.0 if exact else 1e-14), (k, float(t.grad.abs().max()))
