"""Training of the edge-gated cell in the small-graph regime (csrc/gcrnn_small_edge_bwd.hip, ops.small_edge_cell_train,
GGCRNNCell._use_small_edge_training): the forward of the inference path with every state kept, BPTT in two launches.

Gradient reference: oracle/torch_reference.py::ggcrnn_cell under CPU fp64 autograd. Bounds are the project's standing ones (TOLS of
tests/test_fp64_envelopes.py): states max-abs <= 1e-11 (fp64) / 1e-5 (fp32); every gradient max-abs error / max|ref| <= 1e-10 / 2e-5.
"Path taken" is checked with a call counter on the library's entry points.

The long-sequence case rand80 (N = 80, F = 32, K = 3) needs 214 KiB of LDS in fp64 by the formula of
gcrnn_small_edge_backward_supported, so fp64 trains it on the composed path (still at the bounds); fp32 (116 KiB) runs the new kernels.
rand80f20 is the same graph and length at F = 20, which the fp64 kernels accept: 200 steps of the carried dh and of the register-held
folded-tap gradients at the fp64 bounds, on the new path.
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
F32, F64 = 0, 1                                       # dtype codes of include/gcrnn.h
BWD, FWD = 'gcrnn_small_edge_backward', 'gcrnn_small_edge_forward'
COMPOSED = ('gcrnn_attention_forward', 'gcrnn_attention_backward', 'gcrnn_taps_forward')


def gml():
    import gated_gcrnns_amd.Utils.graphML as m
    return m


def archit():
    import gated_gcrnns_amd.Modules.architectures as m
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
    monkeypatch.delenv('GCRNN_NO_SMALL_EDGE', raising=False)
    return s


def new_path_only(spy, backwards=1):
    assert spy.calls[BWD] == backwards, dict(spy.calls)
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
CASES = {'quake':   (gso_adj59, 1, 20, 4, 4, 20, 3, True),
         'kstep':   (gso_sbm50, 1, 20, 5, 5, 5, 4, True),
         'dir17':   (gso_dir17, 3, 7, 3, 2, 3, 2, True),
         'rand80':  (gso_rand80, 1, 32, 3, 3, 200, 2, True),
         'rand80f20': (gso_rand80, 1, 20, 3, 3, 200, 2, True),
         'k1':      (gso_dir17, 3, 7, 1, 1, 3, 2, True),
         'nobias':  (gso_dir17, 3, 7, 3, 2, 3, 2, False)}
_REFS = {}


def make_cell(S, G, F, Kin, Kst, tg, bias, seed, sg='edge', E=1):
    torch.manual_seed(seed)
    cell = gml().GGCRNNCell(G, F, Kin, Kst, torch.tanh, tg, sg, E, bias)
    cell.addGSO(torch.tensor(S))
    return cell.double()


def reference(cell, S, X, h0, Rw, forward):
    """(H, {parameter name or 'h0': gradient}) of loss = (H * Rw).sum() under CPU fp64 autograd; forward(params, S, X, h0) -> H."""
    params = {k: v.detach().clone().requires_grad_() for k, v in cell.state_dict().items()}
    h0t = torch.tensor(h0, requires_grad=True)
    H = forward(params, torch.tensor(S), torch.tensor(X), h0t)
    (H * torch.tensor(Rw)).sum().backward()
    grads = {k: v.grad.detach() for k, v in params.items() if v.grad is not None}
    grads['h0'] = h0t.grad.detach()
    return H.detach(), grads


def case(name, tg):
    """(fp64 cell on the CPU, S, X, h0, R, reference H, reference gradients) -- computed once per (case, gating), never changed."""
    key = (name, tg)
    if key not in _REFS:
        mk, G, F, Kin, Kst, T, B, bias = CASES[name]
        S = mk()
        N = S.shape[1]
        rng = np.random.default_rng(len(name) + 7 * T)
        cell = make_cell(S, G, F, Kin, Kst, tg, bias, seed=T + N)
        X = rng.standard_normal((B, T, G, N))
        h0 = np.tanh(rng.standard_normal((B, F, N)))
        Rw = rng.standard_normal((B, T, F, N))
        H, grads = reference(cell, S, X, h0, Rw, lambda p, S_, X_, h_: tr.ggcrnn_cell(p, S_, X_, h_, time_gating=tg, spatial_gating='edge'))
        _REFS[key] = (cell, S, X, h0, Rw, H, grads)
    return _REFS[key]


def run_cell(cell, X, h0, Rw, dt, dev, x_grad=False):
    """One training step of loss = (H * Rw).sum() on the device: (H, {name or 'h0': gradient})."""
    cell = copy.deepcopy(cell).to(dev).to(dt)
    Xd, hd = Tn(X, dt, dev).requires_grad_(x_grad), Tn(h0, dt, dev).requires_grad_()
    H = cell(Xd, hd)
    (H * Tn(Rw, dt, dev)).sum().backward()
    grads = {k: p.grad for k, p in cell.named_parameters() if p.grad is not None}
    grads['h0'] = hd.grad
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


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('code', [F32, F64])
def test_backward_supported_query_cpu(code):
    from gated_gcrnns_amd._lib import lib
    from gated_gcrnns_amd.graph import GraphOperator
    for S, K in ((gso_adj59(), 4), (gso_sbm50(), 5)):
        op = GraphOperator(S)
        N = S.shape[1]
        assert lib.gcrnn_small_edge_backward_supported(code, N, op.fwd[0].nnz, op.mask.nnz, 1, 20, K, K) == 1
    op = GraphOperator(gso_rand80())                                                             # the long-sequence cases
    assert lib.gcrnn_small_edge_backward_supported(code, 80, op.fwd[0].nnz, op.mask.nnz, 1, 20, 3, 3) == 1
    assert lib.gcrnn_small_edge_backward_supported(code, 80, op.fwd[0].nnz, op.mask.nnz, 1, 32, 3, 3) == int(code == F32)
    assert lib.gcrnn_small_edge_backward_supported(code, 1000, 10000, 11000, 1, 20, 4, 4) == 0
    assert lib.gcrnn_small_edge_backward_supported(code, 200, 2000, 2200, 1, 64, 3, 3) == 0
    assert lib.gcrnn_small_edge_backward_supported(2, 59, 590, 649, 1, 20, 4, 4) == 0            # bf16


def test_backward_supported_is_the_documented_formula_cpu():
    """The LDS formula of include/gcrnn.h, evaluated here, decides at the edge: adj59-like shapes with growing K until it says no."""
    from gated_gcrnns_amd._lib import lib
    N, nnz, nnzs, G, F = 59, 590, 649, 1, 20
    for code, e in ((F32, 4), (F64, 8)):
        for K in range(1, 12):
            C, R = max(G, F), F + 2
            lds = e * (K * C * N + R * K * C + R + 2 * R * N + 3 * N + 3 * nnzs + 2 * nnz + 2 * C * N + 16) + 4 * (4 * (N + 1) + 2 * nnz + 4 * nnzs) + 16
            want = int(lds <= 150 * 1024 and R * (K * C + 1) <= 4096 and lib.gcrnn_small_edge_supported(code, N, nnz, nnzs, G, F, K, K) == 1)
            assert lib.gcrnn_small_edge_backward_supported(code, N, nnz, nnzs, G, F, K, K) == want, (code, K)


def test_backward_argument_validation_cpu():
    """Null pointer, bad shape, bad dtype and unsupported come back as status codes before anything is launched (the pointers
    here are host memory: a launch would be an error of its own)."""
    import ctypes as C
    from gated_gcrnns_amd._lib import lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    BAD_DTYPE, BAD_SHAPE, NULLP, UNSUPPORTED = (lib.gcrnn_status_string(c).decode() for c in (1, 2, 3, 4))     # include/gcrnn.h

    def call(dtype=F64, ptrs=None, B=2, T=3, N=5, G=1, F=4, Kin=2, Kst=2, nnz=6, nnzs=9):
        ptrs = [p] * 33 if ptrs is None else ptrs
        return lib.gcrnn_small_edge_backward(dtype, *ptrs, B, T, N, G, F, Kin, Kst, nnz, nnzs, None)

    def name(status):
        return lib.gcrnn_status_string(status).decode()
    optional = {6, 11, 12, 30, 31, 32}                                       # bias, gi, gf, dgi, dgf, dh0
    for i in range(33):
        if i in optional:
            continue
        ptrs = [p] * 33
        ptrs[i] = None
        assert name(call(ptrs=ptrs)) == NULLP, i
    ptrs = [p] * 33
    ptrs[11] = None                                                        # gi without gf
    assert name(call(ptrs=ptrs)) == NULLP
    ptrs = [p] * 33
    ptrs[30] = None                                                        # gates without a place for their gradient
    assert name(call(ptrs=ptrs)) == NULLP
    ptrs = [p] * 33
    for i in optional:
        ptrs[i] = None                                                     # all optional: the next check answers
    assert name(call(ptrs=ptrs, B=0)) == BAD_SHAPE
    assert name(call(T=0)) == BAD_SHAPE
    assert name(call(N=-1)) == BAD_SHAPE
    assert name(call(B=2 ** 31, T=2)) == BAD_SHAPE
    assert name(call(dtype=2)) == BAD_DTYPE
    assert name(call(dtype=7)) == BAD_DTYPE
    assert name(call(N=1000, F=20, nnz=5000, nnzs=6000)) == UNSUPPORTED
    assert name(call(N=80, F=32, Kin=3, Kst=3, nnz=640, nnzs=720)) == UNSUPPORTED      # fits the forward's LDS, not the backward's
    assert len({NULLP, BAD_SHAPE, BAD_DTYPE, UNSUPPORTED}) == 4


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
    h0 = Tn(g['h0'], dt, dev).requires_grad_()
    H = cell(Tn(g['X'], dt, dev), h0)
    (H.sum() if loss == 'sum' else torch.nn.L1Loss()(H, Tn(g['target'], dt, dev))).backward()
    gref = dict(g['grad_' + loss])
    gref['h0'] = g['grad_%s_h0' % loss]
    grads = {k: p.grad for k, p in cell.named_parameters() if p.grad is not None}
    grads['h0'] = h0.grad
    assert {k for k in g['params'] if not k.startswith(('GFL_out', 'MLP_out'))} <= set(gref)      # every parameter the cell uses
    check_all(H.detach(), grads, torch.tensor(g['H']), gref, dt, 'fixture g3_cell_%s %s' % (name, loss))
    new_path_only(spy)
    assert spy.calls[FWD] == 1


# ---------------------------------------------------------------------------------------------- 2. torch reference
@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('name', ['dir17', 'k1', 'nobias', 'quake', 'kstep'])
def test_against_torch_reference(dev, spy, name, tg, dt):
    cell, S, X, h0, Rw, Href, gref = case(name, tg)
    H, grads = run_cell(cell, X, h0, Rw, dt, dev)
    names = {k for k, _ in cell.named_parameters()}
    if tg:                                                                # (GFL_out / MLP_out are built but never used)
        assert {'GFL_in.weight_A', 'GFL_forget.weight_B', 'MLP_in.0.weight', 'MLP_forget.0.weight'} <= set(gref)
    assert {k for k in names if not k.startswith(('GFL_out', 'MLP_out'))} | {'h0'} == set(gref)
    check_all(H, grads, Href, gref, dt, 'reference %s time_gating=%s' % (name, tg))
    new_path_only(spy)


# ---------------------------------------------------------------------------------------------- 3. long sequence
@pytest.mark.gpu
def test_long_sequence_fp64(dev, spy):
    cell, S, X, h0, Rw, Href, gref = case('rand80', False)
    H, grads = run_cell(cell, X, h0, Rw, torch.float64, dev)
    print('rand80 fp64: %s' % ('new kernels' if spy.calls[BWD] else 'composed path (backward LDS above the limit)'))
    check_all(H, grads, Href, gref, torch.float64, 'rand80 T=200')


@pytest.mark.gpu
def test_long_sequence_fp64_on_the_new_kernels(dev, spy):
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
    monkeypatch.setenv('GCRNN_NO_SMALL_EDGE', '1')
    Hc, gcomp = run_cell(cell, X, h0, Rw, dt, dev)
    assert spy.calls[BWD] == 1 and spy.calls['gcrnn_attention_backward'] > 0
    e_new, e_old = float((H.double().cpu() - Href).abs().max()), float((Hc.double().cpu() - Href).abs().max())
    print('rand80 fp32 states: new %.3e composed %.3e' % (e_new, e_old))
    assert e_new <= max(1e-5, 2 * e_old)
    for k in sorted(gref):
        e_new, e_old = rel_err(grads[k], gref[k]), rel_err(gcomp[k], gref[k])
        print('rand80 fp32 grad %s: new %.3e composed %.3e' % (k, e_new, e_old))
        assert e_new <= max(2e-5, 2 * e_old), k


# ---------------------------------------------------------------------------------------------- 4. determinism
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
    assert torch.equal(H1, H2) and set(g1) == set(g2) and len(g1) >= 8
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for b in (0, 3):
        _, gb = run_cell(cell, X[b:b + 1], h0[b:b + 1], Rw[b:b + 1], dt, dev)
        assert torch.equal(gb['h0'][0], g1['h0'][b]), b
    new_path_only(spy, backwards=4)


# ---------------------------------------------------------------------------------------------- 5. switch and boundaries
def _attention_reference(gate):
    """The edge-gated cell with another attention read-out: gate(raw attention B x K x F x N) -> B x F x N."""
    def forward(params, S, X, h0):
        A, Bw, b = params['weight_A'], params['weight_B'], params.get('bias')
        h, out = h0, []
        for t in range(X.shape[1]):
            ya = gate(tr.graph_attention(tr.lsigf(A, S, X[:, t], b), params['input_attention.mixer'], params['input_attention.weight'], S))
            yb = gate(tr.graph_attention(tr.lsigf(Bw, S, h, b), params['forget_attention.mixer'], params['forget_attention.weight'], S))
            h = torch.tanh(ya + yb)
            out.append(h)
        return torch.stack(out, dim=1)
    return forward


def _edge_reference(params, S, X, h0):
    return tr.ggcrnn_cell(params, S, X, h0, spatial_gating='edge')


def _boundary(name):
    """(fp64 cell on the CPU, S, reference forward, environment, X wants a gradient): every one must stay on the composed path."""
    S17 = gso_dir17()
    G, F, K = 3, 7, 2
    if name in ('switch', 'x_grad'):
        return make_cell(S17, G, F, K, K, False, True, seed=6), S17, _edge_reference, name == 'switch', name == 'x_grad'
    if name == 'refused_shape':
        rng = np.random.default_rng(200)
        S = (rng.random((200, 200)) < 0.03) * rng.uniform(0.1, 1.0, (200, 200))
        S = (S / np.abs(S).sum(axis=1).max()).reshape(1, 200, 200)
        return make_cell(S, 1, 64, 2, 2, False, True, seed=1), S, _edge_reference, False, False
    if name == 'two_heads':
        cell = make_cell(S17, G, F, K, K, False, True, seed=2)
        for att in ('input_attention', 'forget_attention'):
            a = gml().GraphAttentional(F, F, 2, 1, torch.nn.functional.relu, False)            # two heads, averaged
            a.addGSO(cell.graph)
            setattr(cell, att, a.double())
        return cell, S17, _attention_reference(lambda y: torch.relu(y.mean(dim=1))), False, False
    if name == 'tanh_attention':
        cell = make_cell(S17, G, F, K, K, False, True, seed=3)
        cell.input_attention.nonlinearity = torch.tanh
        cell.forget_attention.nonlinearity = torch.tanh
        return cell, S17, _attention_reference(lambda y: torch.tanh(y[:, 0])), False, False
    assert name == 'two_edge_features'
    S2 = np.concatenate([S17, np.transpose(gso_dir17(), (0, 2, 1)) * 0.5], axis=0)           # E = 2
    cell = make_cell(S2, G, F, K, K, False, True, seed=4, sg=None, E=2)
    cell.spatial_gating = 'edge'
    for att in ('input_attention', 'forget_attention'):
        a = gml().GraphAttentional(F, F, 1, 2)
        a.addGSO(cell.graph)
        setattr(cell, att, a.double())
    return cell, S2, _edge_reference, False, False


@pytest.mark.gpu
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', ['switch', 'x_grad', 'refused_shape', 'two_heads', 'tanh_attention', 'two_edge_features'])
def test_boundaries_keep_the_composed_path(dev, spy, monkeypatch, name, dt):
    cell, S, forward, switch, x_grad = _boundary(name)
    N = S.shape[1]
    rng = np.random.default_rng(9)
    X, h0 = rng.standard_normal((2, 2, cell.G, N)), np.tanh(rng.standard_normal((2, cell.F, N)))
    Rw = rng.standard_normal((2, 2, cell.F, N))
    Href, gref = reference(cell, S, X, h0, Rw, forward)
    if switch:
        monkeypatch.setenv('GCRNN_NO_SMALL_EDGE', '1')
    H, grads = run_cell(cell, X, h0, Rw, dt, dev, x_grad=x_grad)
    check_all(H, grads, Href, gref, dt, 'boundary %s' % name)
    assert spy.calls[BWD] == 0 and spy.calls[FWD] == 0, dict(spy.calls)


# ---------------------------------------------------------------------------------------------- 6. capture
@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
def test_training_step_captures_under_cuda_graph(dev, spy, tg):
    dt = torch.float32
    S = gso_sbm50()
    torch.manual_seed(50)
    m = archit().GatedGCRNNforRegression(1, 20, 5, 5, torch.tanh, torch.nn.ReLU, [1], S[0], True,
                                         time_gating=tg, spatial_gating='edge', mlpType='multipMlp').to(dev).to(dt)
    rng = np.random.default_rng(50)
    x, h0 = Tn(rng.standard_normal((4, 5, 1, 50)), dt, dev), torch.zeros((4, 20, 50), dtype=dt, device=dev)
    params = [p for p in m.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        y = m(x, h0)
        y.abs().mean().backward()
    step()                                                    # eager (and warm-up: the graph's plans are built here)
    want = [p.grad.clone() if p.grad is not None else None for p in params]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(s)
    before = spy.calls[BWD]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    assert spy.calls[BWD] == before + 1
    got = [p.grad for p in params]
    for t in got:
        if t is not None:
            t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert sum(w is not None for w in want) >= 9
    for w, t in zip(want, got):
        assert (w is None) == (t is None)
        if w is not None:
            assert torch.equal(w, t)
    for name in COMPOSED:
        assert spy.calls[name] == 0
    del g


# ---------------------------------------------------------------------------------------------- 7. models
def _three_adam_steps(model, x, h0, target, dev):
    from gated_gcrnns_amd.optim import FlatAdam
    m = copy.deepcopy(model).to(dev)
    opt = FlatAdam(m.parameters(), lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        (m(x, h0) - target).square().mean().backward()
        opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('kind', ['classification', 'regression'])
def test_models_train_as_on_the_composed_path(dev, spy, monkeypatch, kind, tg):
    """Three FlatAdam steps (lr = 1e-3) on the new path against three on the composed path, fp64: parameters agree to 1e-9 max-abs (the
    updates amplify the 1e-10 gradient bound by less than 10)."""
    dt = torch.float64
    rng = np.random.default_rng(59)
    torch.manual_seed(59)
    if kind == 'classification':
        S = gso_adj59()
        m = archit().GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [11], S[0], True,
                                                 time_gating=tg, spatial_gating='edge').double()
        x, h0 = Tn(rng.standard_normal((3, 20, 1, 59)), dt, dev), torch.zeros((3, 20, 59), dtype=dt, device=dev)
    else:
        S = gso_sbm50()
        m = archit().GatedGCRNNforRegression(1, 20, 5, 5, torch.tanh, torch.nn.ReLU, [1], S[0], True,
                                             time_gating=tg, spatial_gating='edge', mlpType='multipMlp').double()
        x, h0 = Tn(rng.standard_normal((4, 5, 1, 50)), dt, dev), torch.zeros((4, 20, 50), dtype=dt, device=dev)
    with torch.no_grad():
        shape = copy.deepcopy(m).to(dev)(x, h0).shape
    target = Tn(rng.standard_normal(tuple(shape)), dt, dev)
    new = _three_adam_steps(m, x, h0, target, dev)
    new_path_only(spy, backwards=3)
    monkeypatch.setenv('GCRNN_NO_SMALL_EDGE', '1')
    old = _three_adam_steps(m, x, h0, target, dev)
    assert spy.calls[BWD] == 3 and spy.calls['gcrnn_attention_backward'] > 0
    start = dict(m.named_parameters())
    moved = 0
    for k in new:
        err = float((new[k] - old[k]).abs().max())
        assert err <= 1e-9, (k, err)
        moved += int(float((new[k].cpu() - start[k].detach()).abs().max()) > 1e-4)
    print('%s time_gating=%s: %d of %d parameters moved' % (kind, tg, moved, len(new)))
    assert moved >= 8
