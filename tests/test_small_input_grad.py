"""GPU (-m gpu): input gradients (dX) of the one-launch small-graph BPTT kernels -- the dx variants of small_cell_bwd_kernel (gather family),
small_dense_bwd_kernel (matrix-core family, per-node gates included) and small_gate_bwd_kernel (time gates) -- against the reference's
fixtures and the plain-torch fp64 reference (oracle/torch_reference.py, autograd).

Tolerances are the project's (TOLS of test_fp64_envelopes.py): fp64 states <= 1e-11, gradients <= 1e-10 of their own
maximum; fp32 states <= 1e-5, gradients <= 2e-5. Every case counts the library's entry points (wrapper around ops.lib): the dx entry point
of the family ran exactly once per backward, the plain one not at all, so no case can pass on the composed path. Graphs, initialisation and
the counting wrapper follow test_fp64_envelopes.py.

On the gather family the time gates are composed (lsigf on gcrnn_taps_*, already differentiable in X), so gcrnn_taps_* does run for a
time-gated cell there; those cases assert instead that neither the gates' kernels nor the matrix-core kernels ran. On the matrix-core
family no gcrnn_taps_* call is made for un-gated and time-gated cells; the node gates stay on their composed pass."""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import torch_reference as tr

pytestmark = pytest.mark.gpu

D_FWD, D_BWD, D_DX = 'gcrnn_small_dense_forward', 'gcrnn_small_dense_backward', 'gcrnn_small_dense_backward_dx'
S_FWD, S_BWD, S_DX = 'gcrnn_small_forward', 'gcrnn_small_backward', 'gcrnn_small_backward_dx'
GT_FWD, GT_BWD, GT_DX = 'gcrnn_small_gates_forward', 'gcrnn_small_gates_backward', 'gcrnn_small_gates_backward_dx'
TAPS3 = ('gcrnn_taps_forward', 'gcrnn_taps_backward_data', 'gcrnn_taps_backward_weight')
ATT_F, ATT_B = 'gcrnn_attention_forward', 'gcrnn_attention_backward'
SMALL = (D_FWD, D_BWD, D_DX, S_FWD, S_BWD, S_DX, GT_FWD, GT_BWD, GT_DX)
TOLS = {torch.float64: (1e-11, 1e-10), torch.float32: (1e-5, 2e-5)}
DTS = (torch.float64, torch.float32)


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


class _CountingLib(object):
    """ops.lib with a call counter on every compute entry point (queries -- *_supported, *_parts, *_slots, *_blocks -- pass through)."""

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


def set_family(monkeypatch, gather):
    if gather:
        monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')
    else:
        monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)


@functools.lru_cache(maxsize=None)
def graph(N, seed, uniform=False):
    """1 x N x N GSO, spectral radius 1. Directed, weights in +-[0.2, 1] (one weight everywhere when uniform); node 0 isolated, node 1 a hub
    with >= N/4 out- and in-neighbours, self-loops on N/8 nodes."""
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
    if not uniform:
        M *= rng.uniform(0.2, 1.0, (N, N)) * rng.choice([-1.0, 1.0], (N, N), p=[0.3, 0.7])
    M /= np.max(np.abs(np.linalg.eigvals(M)))
    S = M[None]
    if N >= 8:
        assert not np.allclose(S, S.transpose(0, 2, 1)) and np.count_nonzero(S[0, 1]) >= N / 4 and np.count_nonzero(S[0, :, 1]) >= N / 4
    return S


def _init(cell, G, F, Ki, Ks, E=1):
    """Taps at 1/sqrt(fan-in) (a contracting recurrence: fp32 noise is not amplified over T = 200 steps); read-outs of the time gates and the
    node gates' filters scaled up so that the gates are far from 0.5."""
    with torch.no_grad():
        for name, p in cell.named_parameters():
            if name.endswith('weight_A'):
                p.uniform_(-1.0, 1.0).mul_(1.0 / np.sqrt(G * Ki * E))
            elif name.endswith('weight_B'):
                p.uniform_(-1.0, 1.0).mul_(1.0 / np.sqrt(F * Ks * E))
            elif name.startswith('MLP_'):
                p.mul_(6.0)
            elif name.startswith('GFL_node_'):
                p.mul_(3.0)
            elif name.endswith('attention.mixer'):
                p.mul_(4.0)
    ops().parameters_changed()


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _close(got, ref, tol, what):
    err = _rel(got, ref)
    print('%s: %.3g' % (what, err))
    assert err <= tol, '%s: %.3g of its maximum' % (what, err)
    return err


def _abs_close(got, ref, tol, what):
    err = float((got.double() - ref).abs().max())
    print('%s: %.3g' % (what, err))
    assert err <= tol, '%s: %.3g' % (what, err)


def expected_calls(gather, tg, sg, fwd_dense=True):
    """(entry points that run exactly once per forward + backward, entry points that must not run) with X requiring grad. fwd_dense:
    the forward runs on the matrix-core family too (its LDS image, every hop level of z, is the larger one: at the backward's LDS edge
    the forward is the gather kernel's)."""
    if gather:
        once, never = (S_FWD, S_DX), (S_BWD, D_FWD, D_BWD, D_DX, GT_FWD, GT_BWD, GT_DX)
        if not tg:
            never += TAPS3
        return once, never
    once, never = (D_FWD, D_DX), (D_BWD, S_FWD, S_BWD, S_DX, GT_BWD)
    if not fwd_dense:
        once, never = (S_FWD, D_DX), (D_BWD, D_FWD, S_BWD, S_DX, GT_BWD)
    if tg:
        once += (GT_FWD, GT_DX)
    else:
        never += (GT_FWD, GT_DX)
    if sg is None:
        never += TAPS3          # the node gates themselves stay on their composed pass (gcrnn_taps_*)
    return once, never


def assert_calls(spy, once, never, what):
    for name in once:
        assert spy.calls[name] == 1, '%s: %s ran %d times (%s)' % (what, name, spy.calls[name], dict(spy.calls))
    for name in never:
        assert spy.calls[name] == 0, '%s: %s ran (%s)' % (what, name, dict(spy.calls))


def make_cell(N, G, F, Ki, Ks, tg, sg, uniform=False, bias=True, seed_extra=0):
    S = graph(N, 1000 + N + 7 * F, uniform)
    torch.manual_seed(N + F + seed_extra)
    cell = gml().GGCRNNCell(G, F, Ki, Ks, torch.tanh, tg, sg, 1, bias)
    cell.addGSO(torch.tensor(S))
    cell = cell.double()
    _init(cell, G, F, Ki, Ks)
    return cell, S


def run_case(dev, spy, monkeypatch, N, G, F, Ki, Ks, B, T, tg=False, sg=None, uniform=False, gather=False, bias=True, frozen=False,
             h0_grad=True, view=False):
    """The cell with X (and, unless stated, h0 and every parameter) requiring grad, loss (H * R).sum(), both dtypes, against torch_reference.
    Returns {dtype: dX} of the kernels."""
    set_family(monkeypatch, gather)
    cell, S = make_cell(N, G, F, Ki, Ks, tg, sg, uniform, bias)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64).to(dev)
    h0 = (0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64)).to(dev)
    R = torch.randn(B, T, F, N, generator=gen, dtype=torch.float64).to(dev)
    Sd = torch.tensor(S, device=dev)
    rp = {k: v.detach().to(dev).clone().requires_grad_(not frozen) for k, v in cell.state_dict().items()}
    Xr, h0r = X.clone().requires_grad_(True), h0.clone().requires_grad_(h0_grad)
    Hr = tr.ggcrnn_cell(rp, Sd, Xr, h0r, tg, sg)
    (Hr * R).sum().backward()
    nnz = int(np.count_nonzero(S[0]))
    out = {}
    for dt in DTS:
        stol, gtol = TOLS[dt]
        once, never = expected_calls(gather, tg, sg, ops().small_dense_supported(N, G, F, Ki, Ks, dt, backward=False,
                                                                                  gated=tg or sg is not None))
        assert ops().small_input_grad_supported(N, nnz, G, F, Ki, Ks, dt, 1, gated=tg or sg is not None, node_gates=sg is not None)
        cd = copy.deepcopy(cell).to(dev).to(dt)
        for p in cd.parameters():
            p.requires_grad_(not frozen)
        if view:      # X as a non-contiguous view: [B][T][N][G] storage seen as [B][T][G][N]
            Xd = X.to(dt).transpose(2, 3).contiguous().requires_grad_(True)
            Xin = Xd.transpose(2, 3)
            assert not Xin.is_contiguous() or G == 1 or N == 1
        else:
            Xd = X.to(dt).clone().requires_grad_(True)
            Xin = Xd
        h0d = h0.to(dt).clone().requires_grad_(h0_grad)
        spy.calls.clear()
        H = cd(Xin, h0d)
        (H * R.to(dt)).sum().backward()
        torch.cuda.synchronize()
        assert_calls(spy, once, never, str(dt))
        assert H.dtype == dt and tuple(H.shape) == (B, T, F, N)
        _abs_close(H.detach(), Hr.detach(), stol, '%s states' % dt)
        got = dict(cd.named_parameters())
        for k, v in rp.items():
            if v.grad is None or float(v.grad.abs().max()) == 0.0:
                assert got[k].grad is None or float(got[k].grad.abs().max()) == 0.0, k
                continue
            assert got[k].grad is not None, '%s: no gradient for %s' % (dt, k)
            _close(got[k].grad, v.grad, gtol, '%s grad %s' % (dt, k))
        if h0_grad:
            _close(h0d.grad, h0r.grad, gtol, '%s grad h0' % dt)
        else:
            assert h0d.grad is None
        assert Xd.grad is not None, '%s: no gradient for X' % dt
        dX = Xd.grad.transpose(2, 3) if view else Xd.grad
        assert tuple(dX.shape) == (B, T, G, N)
        _close(dX, Xr.grad, gtol, '%s grad X' % dt)      # T = 200 in fp32 included: measured 4.8e-7 at most
        out[dt] = dX.detach().clone()
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. reference fixtures
FIXTURES = [('none', False, None, False), ('none', False, None, True), ('time', True, None, False), ('time', True, None, True),
            ('node', False, 'node', False), ('time_node', True, 'node', False)]


def _relnp(t, ref):
    return float(np.max(np.abs(t.detach().double().cpu().numpy() - ref)) / (np.max(np.abs(ref)) + 1e-30))


@pytest.mark.parametrize('dt', DTS, ids=['fp64', 'fp32'])
@pytest.mark.parametrize('name,tg,sg,gather', FIXTURES, ids=['%s-%s' % (f[0], 'gather' if f[3] else 'mfma') for f in FIXTURES])
def test_reference_fixtures(dev, spy, monkeypatch, name, tg, sg, gather, dt):
    """g3_cell_* (N = 30, G = 2, F = 5, K = 3, B = 3, T = 4): dX, dh0 and the parameter gradients of both losses the fixtures store."""
    set_family(monkeypatch, gather)
    g = load_golden('g3_cell_' + name)
    stol, gtol = TOLS[dt]
    cell = gml().GGCRNNCell(2, 5, 3, 3, torch.tanh, tg, sg, 1, True)
    cell.addGSO(torch.tensor(g['S']))
    cell = cell.double()
    cell.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    cell = cell.to(dev).to(dt)
    ops().parameters_changed()
    X = torch.tensor(g['X'], dtype=dt, device=dev, requires_grad=True)
    h0 = torch.tensor(g['h0'], dtype=dt, device=dev, requires_grad=True)
    once, never = expected_calls(gather, tg, sg)
    spy.calls.clear()
    H = cell(X, h0)
    assert float(np.max(np.abs(H.detach().double().cpu().numpy() - g['H']))) <= stol
    H.sum().backward()
    torch.cuda.synchronize()
    assert_calls(spy, once, never, 'sum loss')
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
    assert_calls(spy, once, never, 'L1 loss')
    for k, p in cell.named_parameters():
        ref = g['grad_l1'].get(k)
        if ref is not None:
            assert _relnp(p.grad, ref) <= gtol, k
    assert _relnp(X.grad, g['grad_l1_X']) <= gtol


# ---------------------------------------------------------------------------------------------------------------- 2. matrix-core family
def shape(cid, N, G, F, Ki, Ks, B, T, **kw):
    return pytest.param(dict(N=N, G=G, F=F, Ki=Ki, Ks=Ks, B=B, T=T, **kw), id=cid)


DENSE = [
    shape('N1', 1, 1, 1, 1, 1, 3, 4),
    shape('K1-no-hops', 30, 3, 20, 1, 1, 2, 4),
    shape('K5', 40, 2, 12, 5, 5, 2, 3),
    shape('node-Kin>Kst', 40, 3, 12, 3, 2, 2, 3, sg='node'),
    shape('time-node', 33, 2, 8, 2, 2, 2, 3, tg=True, sg='node'),
    shape('time-tile-edges-N65-F33', 65, 1, 33, 1, 1, 2, 3, tg=True),
    shape('time-G63', 24, 63, 16, 2, 2, 2, 3, tg=True),
    shape('time-G1-K5', 20, 1, 8, 5, 5, 2, 3, tg=True),
    shape('uniform-T200', 24, 2, 8, 2, 2, 2, 200, uniform=True),
]


@pytest.mark.parametrize('c', DENSE)
def test_matrix_core_family(c, dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, **c)


# ---------------------------------------------------------------------------------------------------------------- 3. gather family
GATHER = [
    shape('K1-B1', 63, 2, 8, 1, 1, 1, 4),
    shape('K2-P4', 64, 1, 32, 2, 2, 2, 3),
    shape('K3-time', 65, 1, 31, 3, 3, 2, 3, tg=True),
    shape('K4-P4', 69, 2, 30, 4, 4, 2, 3),
    shape('K5-B1-T200-uniform', 33, 3, 16, 5, 5, 1, 200, uniform=True),
]


@pytest.mark.parametrize('c', GATHER)
def test_gather_family(c, dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, gather=True, **c)


# ---------------------------------------------------------------------------------------------------------------- 4. LDS edges
def test_matrix_core_lds_edge(dev, spy, monkeypatch):
    """fp64, un-gated, N = 88, G = 8, F = 20: the dx image (dense S, two z buffers, dpre, carry and the taps of BOTH filters for the adjoint
    chain) fits 160 KB with 4 taps per filter and not with 5, while the plain backward (state taps only) still takes 5 -- there a cell
    whose X wants a gradient stays on the composed path."""
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    lib, code = ops().lib, ops().dtype_code(torch.float64)
    N, G, F, K = DENSE_EDGE
    assert lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, K, K, 0) == 1
    assert lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, K + 1, K + 1, 0) == 0
    assert lib.gcrnn_small_dense_supported(code, N, G, F, K + 1, K + 1, 1, 0) == 1
    nnz = int(np.count_nonzero(graph(N, 1000 + N + 7 * F)[0]))
    assert ops().small_training_supported(N, nnz, G, F, K + 1, K + 1, torch.float64)
    assert not ops().small_input_grad_supported(N, nnz, G, F, K + 1, K + 1, torch.float64)
    run_case(dev, spy, monkeypatch, N, G, F, K, K, 2, 3)


def test_gather_lds_edge(dev, spy, monkeypatch):
    """The gather family's dx variant shares the plain backward's image (the adjoint chain runs in the two z buffers), so it has no LDS
    edge of its own: the family's edge is where the kernels' 150 KB end (N = 512, F = 5: four taps fit, five do not), asserted through
    the query -- accepted, and refused with one more tap. F N > 2048: the four-pass instantiation."""
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')
    N, G, F, K = GATHER_EDGE
    nnz = int(np.count_nonzero(graph(N, 1000 + N + 7 * F)[0]))
    for dt in DTS:
        assert ops().small_input_grad_supported(N, nnz, G, F, K, K, dt)
    assert not ops().small_input_grad_supported(N, nnz, G, F, K + 1, K + 1, torch.float64)
    run_case(dev, spy, monkeypatch, N, G, F, K, K, 2, 3, gather=True)


DENSE_EDGE = (88, 8, 20, 4)
GATHER_EDGE = (512, 1, 5, 4)


# ---------------------------------------------------------------------------------------------------------------- 5. variants
BASE = dict(N=40, G=2, F=12, Ki=5, Ks=5, B=2, T=3)


def test_no_bias(dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, bias=False, **BASE)


def test_frozen_parameters_only_x_wants_grad(dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, frozen=True, h0_grad=False, **BASE)


def test_h0_without_grad(dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, h0_grad=False, **BASE)


def test_non_contiguous_x(dev, spy, monkeypatch):
    run_case(dev, spy, monkeypatch, view=True, **BASE)


@pytest.mark.parametrize('tg,sg,gather', [(False, None, False), (True, None, False), (False, 'node', False), (False, None, True)],
                         ids=['none', 'time', 'node', 'gather'])
def test_dx_is_bit_identical_between_runs(dev, spy, monkeypatch, tg, sg, gather):
    a = run_case(dev, spy, monkeypatch, tg=tg, sg=sg, gather=gather, **BASE)
    b = run_case(dev, spy, monkeypatch, tg=tg, sg=sg, gather=gather, **BASE)
    for dt in DTS:
        assert torch.equal(a[dt], b[dt]), dt


# ---------------------------------------------------------------------------------------------------------------- 6. ops level
@pytest.mark.parametrize('gather', [False, True], ids=['mfma', 'gather'])
def test_ops_small_cell_train_returns_dx(dev, spy, monkeypatch, gather):
    from gated_gcrnns_amd.graph import GraphOperator
    set_family(monkeypatch, gather)
    N, G, F, K, B, T = 30, 2, 5, 3, 2, 4
    S = graph(N, 77)
    gop = GraphOperator(S, device=dev)
    gen = torch.Generator().manual_seed(3)
    wA = (torch.rand(F, 1, K, G, generator=gen, dtype=torch.float64) * 2 - 1) / np.sqrt(G * K)
    wB = (torch.rand(F, 1, K, F, generator=gen, dtype=torch.float64) * 2 - 1) / np.sqrt(F * K)
    bias = torch.rand(F, 1, generator=gen, dtype=torch.float64) - 0.5
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64)
    h0 = 0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64)
    R = torch.randn(B, T, F, N, generator=gen, dtype=torch.float64)
    rp = {'weight_A': wA.to(dev).requires_grad_(True), 'weight_B': wB.to(dev).requires_grad_(True), 'bias': bias.to(dev).requires_grad_(True)}
    Xr, h0r = X.to(dev).requires_grad_(True), h0.to(dev).requires_grad_(True)
    (tr.ggcrnn_cell(rp, torch.tensor(S, device=dev), Xr, h0r) * R.to(dev)).sum().backward()
    for dt in DTS:
        stol, gtol = TOLS[dt]
        a, bq, c = (t.to(dev).to(dt).requires_grad_(True) for t in (wA, wB, bias))
        Xd, h0d = X.to(dev).to(dt).requires_grad_(True), h0.to(dev).to(dt).requires_grad_(True)
        spy.calls.clear()
        H = ops().small_cell_train(Xd, h0d, a, bq, c, gop)
        (H * R.to(dev).to(dt)).sum().backward()
        torch.cuda.synchronize()
        assert spy.calls[S_DX if gather else D_DX] == 1 and spy.calls[S_BWD] == 0 and spy.calls[D_BWD] == 0, dict(spy.calls)
        assert Xd.grad is not None
        _close(Xd.grad, Xr.grad, gtol, '%s grad X' % dt)
        _close(h0d.grad, h0r.grad, gtol, '%s grad h0' % dt)
        _close(a.grad, rp['weight_A'].grad, gtol, '%s grad wA' % dt)
        _close(bq.grad, rp['weight_B'].grad, gtol, '%s grad wB' % dt)
        _close(c.grad, rp['bias'].grad, gtol, '%s grad b' % dt)


# ---------------------------------------------------------------------------------------------------------------- 7. stacked cells
def test_stacked_cells(dev, spy, monkeypatch):
    """cell2(cell1(X, h0a), h0b): cell2's input is cell1's output, so cell2's backward must return dX; X wants one too."""
    set_family(monkeypatch, False)
    N, G, F1, F2, K, B, T = 30, 2, 5, 4, 3, 2, 4
    S = graph(N, 1000 + N + 7 * F1)
    c1, _ = make_cell(N, G, F1, K, K, False, None)
    torch.manual_seed(99)
    c2 = gml().GGCRNNCell(F1, F2, K, K, torch.tanh, False, None, 1, True)
    c2.addGSO(torch.tensor(S))
    c2 = c2.double()
    _init(c2, F1, F2, K, K)
    gen = torch.Generator().manual_seed(11)
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64).to(dev)
    ha = (0.5 * torch.randn(B, F1, N, generator=gen, dtype=torch.float64)).to(dev)
    hb = (0.5 * torch.randn(B, F2, N, generator=gen, dtype=torch.float64)).to(dev)
    R = torch.randn(B, T, F2, N, generator=gen, dtype=torch.float64).to(dev)
    Sd = torch.tensor(S, device=dev)
    rp1 = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in c1.state_dict().items()}
    rp2 = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in c2.state_dict().items()}
    Xr, har, hbr = (t.clone().requires_grad_(True) for t in (X, ha, hb))
    Hr = tr.ggcrnn_cell(rp2, Sd, tr.ggcrnn_cell(rp1, Sd, Xr, har), hbr)
    (Hr * R).sum().backward()
    for dt in DTS:
        stol, gtol = TOLS[dt]
        d1, d2 = copy.deepcopy(c1).to(dev).to(dt), copy.deepcopy(c2).to(dev).to(dt)
        Xd, had, hbd = (t.to(dt).clone().requires_grad_(True) for t in (X, ha, hb))
        spy.calls.clear()
        H = d2(d1(Xd, had), hbd)
        (H * R.to(dt)).sum().backward()
        torch.cuda.synchronize()
        assert spy.calls[D_FWD] == 2 and spy.calls[D_DX] == 2 and spy.calls[D_BWD] == 0, dict(spy.calls)
        assert not [n for n in spy.calls if n.startswith('gcrnn_taps_')], dict(spy.calls)
        _abs_close(H.detach(), Hr.detach(), stol, '%s states' % dt)
        for cd, rp in ((d1, rp1), (d2, rp2)):
            got = dict(cd.named_parameters())
            for k, v in rp.items():
                if v.grad is None or float(v.grad.abs().max()) == 0.0:
                    continue
                _close(got[k].grad, v.grad, gtol, '%s grad %s' % (dt, k))
        _close(Xd.grad, Xr.grad, gtol, '%s grad X' % dt)
        _close(had.grad, har.grad, gtol, '%s grad h0a' % dt)
        _close(hbd.grad, hbr.grad, gtol, '%s grad h0b' % dt)


def test_cell2_alone_runs_its_dx_entry_point(dev, spy, monkeypatch):
    """The second cell of a stack sees an input that is not a leaf: its backward runs on the dx entry point."""
    set_family(monkeypatch, False)
    cell, S = make_cell(30, 5, 4, 3, 3, False, None)
    cd = cell.to(dev)
    Xmid = torch.randn(2, 4, 5, 30, dtype=torch.float64, device=dev, requires_grad=True) * 1.0
    assert not Xmid.is_leaf
    spy.calls.clear()
    cd(Xmid, torch.zeros(2, 4, 30, dtype=torch.float64, device=dev)).sum().backward()
    assert spy.calls[D_DX] == 1 and spy.calls[D_BWD] == 0, dict(spy.calls)


# ---------------------------------------------------------------------------------------------------------------- 8. fallback guard
def test_edge_gated_cell_keeps_its_path(dev, spy, monkeypatch):
    """Unchanged behaviour: an edge-gated cell whose X wants a gradient runs the attention kernels and none of the small entry points."""
    set_family(monkeypatch, False)
    N, G, F, K, B, T = 40, 3, 6, 2, 2, 3
    S = graph(N, 1000 + N + 7 * F)
    torch.manual_seed(N + F)
    cell = gml().GGCRNNCell(G, F, K, K, torch.tanh, False, 'edge', 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.double()
    _init(cell, G, F, K, K)
    cell = cell.to(dev)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    h0 = (0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64)).to(dev).requires_grad_(True)
    spy.calls.clear()
    cell(X, h0).sum().backward()
    torch.cuda.synchronize()
    ran = set(spy.calls)
    assert ATT_F in ran and ATT_B in ran, sorted(ran)
    assert not [n for n in ran if n in SMALL or n.startswith('gcrnn_small_edge')], sorted(ran)
    assert X.grad is not None
