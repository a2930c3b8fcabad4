"""GPU (-m gpu): every fp64 kernel path that the fp32-vs-fp64 sweeps take as their truth, at the edges of its envelope, against the plain-torch
fp64 reference (oracle/torch_reference.py: dense S, torch's own ops, autograd gradients; pinned to the reference's fixtures by
tests/test_torch_reference.py).

Each case builds the module on a stated path and asserts that the HIP entry points of that path ran and those of the other paths did not (the
library's entry points are counted through a wrapper around ops.lib): no case can pass on a fallback. fp64: states <= 1e-11, every gradient
(parameters, h0, X where wanted) <= 1e-10 of its max. The same case in fp32 on the same reference: states <= 1e-5, gradients <= 2e-5 (DESIGN
section 2) -- the kernels are templates on the element type, so a tile-edge or indexing bug that fp32-vs-fp64 comparisons cannot see shows here.

Graphs are directed and weighted (signs mixed), with an isolated node, a hub whose in- and out-degree are >= N/4 and self-loops; one case per
path runs on a uniform-weight graph (the uniform fast paths). Some edges named by the kernels' predicates cannot be reached in fp64: a dense S
in LDS caps the matrix-core family at N = 120 (fp64) / 180 (fp32), so N = 255 / 256 run on the gather kernels, and tilesF * tilesN = 64
(forward) or = 32 (gated backward) fit no shape that small_supported admits; those cases assert the path that does run and test the largest
shape that is reachable."""
import collections
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import torch_reference as tr

pytestmark = pytest.mark.gpu

D_FWD, D_BWD = 'gcrnn_small_dense_forward', 'gcrnn_small_dense_backward'
S_FWD, S_BWD = 'gcrnn_small_forward', 'gcrnn_small_backward'
GT_FWD, GT_BWD = 'gcrnn_small_gates_forward', 'gcrnn_small_gates_backward'
TAPS, TAPS_MFMA, TBD, TBW = 'gcrnn_taps_forward', 'gcrnn_taps_mfma_forward', 'gcrnn_taps_backward_data', 'gcrnn_taps_backward_weight'
SPMM, SPMM_EX = 'gcrnn_spmm', 'gcrnn_spmm_ex'
ATT_F, ATT_B = 'gcrnn_attention_forward', 'gcrnn_attention_backward'
GFL_F, GFL_B = 'gcrnn_graph_filter_layer_forward', 'gcrnn_graph_filter_layer_backward'
SMALL = (D_FWD, D_BWD, S_FWD, S_BWD, GT_FWD, GT_BWD)
TOLS = {torch.float64: (1e-11, 1e-10), torch.float32: (1e-5, 2e-5)}


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


@functools.lru_cache(maxsize=None)
def graph(N, seed, uniform=False, E=1):
    """E x N x N GSO, spectral radius 1. Directed, weights in +-[0.2, 1] (one weight everywhere when uniform); node 0 isolated, node 1 a hub
    with >= N/4 out- and in-neighbours, self-loops on N/8 nodes."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(E):
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
        out.append(M)
    S = np.stack(out)
    if N >= 8:
        assert not np.allclose(S, S.transpose(0, 2, 1)) and np.count_nonzero(S[0, 1]) >= N / 4 and np.count_nonzero(S[0, :, 1]) >= N / 4
    return S


def case(cid, N, G, F, Ki, Ks, B, T, mode, runs, not_runs=(), tg=False, sg=None, E=1, uniform=False, gather=False, f32=True, extra=None):
    """mode: 'infer' (no_grad), 'train' (gradients for every parameter and h0, none for X) or 'trainx' (for X too). runs / not_runs: entry
    points that must / must not run in fp64 (and in fp32 unless f32 is False: there the fp32 dispatch picks another family)."""
    return pytest.param(dict(N=N, G=G, F=F, Ki=Ki, Ks=Ks, B=B, T=T, mode=mode, runs=runs, not_runs=not_runs, tg=tg, sg=sg, E=E,
                             uniform=uniform, gather=gather, f32=f32, extra=extra or {}), id=cid)


NOT_DENSE = (D_FWD, D_BWD)
NOT_GATHER = (S_FWD, S_BWD)
CASES = [
    # ---- small-graph matrix-core family (dense S in LDS), inference
    case('dense-fwd-N1', 1, 1, 1, 1, 1, 3, 4, 'infer', (D_FWD,), NOT_GATHER),
    case('dense-fwd-N15-Kin>Kst-G17', 15, 17, 16, 6, 3, 2, 3, 'infer', (D_FWD,), NOT_GATHER),
    case('dense-fwd-N16-Kin<Kst-F17', 16, 1, 17, 2, 8, 2, 3, 'infer', (D_FWD,), NOT_GATHER),
    case('dense-fwd-N17-F64-G17', 17, 17, 64, 1, 1, 2, 3, 'infer', (D_FWD,), NOT_GATHER),
    case('dense-fwd-K8', 17, 1, 16, 8, 8, 2, 3, 'infer', (D_FWD,), NOT_GATHER),
    case('dense-fwd-tiles24', 49, 1, 81, 1, 1, 2, 2, 'infer', (D_FWD,), NOT_GATHER, extra=dict(tiles=24)),
    case('dense-fwd-N120-uniform', 120, 1, 16, 2, 2, 2, 3, 'infer', (D_FWD,), NOT_GATHER, uniform=True),
    case('dense-fwd-T200', 20, 2, 8, 3, 3, 2, 200, 'infer', (D_FWD,), NOT_GATHER),
    case('small-fwd-N255-gather', 255, 1, 4, 2, 2, 2, 3, 'infer', (S_FWD,), NOT_DENSE),
    case('small-fwd-N256-gather', 256, 1, 4, 2, 2, 2, 3, 'infer', (S_FWD,), NOT_DENSE),
    # ---- matrix-core BPTT
    case('dense-bptt-KtFtC64', 2, 96, 17, 4, 4, 2, 3, 'train', (D_FWD, D_BWD), NOT_GATHER, extra=dict(wtiles=64)),
    case('dense-bptt-K1', 30, 3, 20, 1, 1, 2, 4, 'train', (D_FWD, D_BWD), NOT_GATHER),
    case('dense-bptt-K5', 40, 2, 12, 5, 5, 2, 3, 'train', (D_FWD, D_BWD), NOT_GATHER),
    case('dense-bptt-gated-tiles15', 65, 1, 33, 1, 1, 2, 3, 'train', (D_FWD, D_BWD), NOT_GATHER, tg=True),
    case('dense-bptt-uniform-T200', 24, 2, 8, 2, 2, 2, 200, 'train', (D_FWD, D_BWD), NOT_GATHER, uniform=True),
    # ---- small time gates (both gates of all steps in one launch)
    case('gates-G1-K8', 20, 1, 8, 8, 8, 2, 3, 'infer', (GT_FWD, D_FWD), NOT_GATHER, tg=True),
    case('gates-G1-K5-bptt', 20, 1, 8, 5, 5, 2, 3, 'train', (GT_FWD, GT_BWD, D_FWD, D_BWD), NOT_GATHER, tg=True),
    case('gates-G63-bptt', 24, 63, 16, 2, 2, 2, 3, 'train', (GT_FWD, GT_BWD, D_FWD, D_BWD), NOT_GATHER, tg=True),
    case('gates-G64-tiles16', 24, 64, 16, 4, 4, 2, 3, 'infer', (GT_FWD, D_FWD), NOT_GATHER, tg=True, extra=dict(gate_tiles=16)),
    case('gates-G64-tiles16-bptt', 24, 64, 16, 4, 4, 2, 3, 'train', (GT_FWD, GT_BWD, D_FWD, D_BWD), NOT_GATHER, tg=True, uniform=True),
    # ---- node-gated small cell (matrix-core family only); N = 256 is beyond it: composed path
    case('node-dense', 40, 3, 12, 3, 2, 2, 3, 'infer', (D_FWD,), NOT_GATHER, sg='node'),
    case('node-dense-bptt', 40, 3, 12, 3, 2, 2, 3, 'train', (D_FWD, D_BWD), NOT_GATHER, sg='node'),
    case('node-time-dense-bptt', 33, 2, 8, 2, 2, 2, 3, 'train', (D_FWD, D_BWD), NOT_GATHER, sg='node', tg=True),
    case('node-N256-composed', 256, 2, 8, 2, 2, 2, 3, 'train', (TAPS, TBD, TBW), SMALL, sg='node'),
    # ---- small-graph gather family (CSR in LDS, GCRNN_SMALL_GATHER=1)
    case('gather-fwd-N257', 257, 2, 8, 3, 3, 2, 3, 'infer', (S_FWD,), NOT_DENSE, gather=True),
    case('gather-fwd-N1023', 1023, 1, 4, 2, 2, 2, 3, 'infer', (S_FWD,), NOT_DENSE, gather=True),
    case('gather-fwd-N1024-FN4096-uniform', 1024, 1, 4, 2, 2, 2, 3, 'infer', (S_FWD,), NOT_DENSE, gather=True, uniform=True),
    case('gather-fwd-LDS-edge', 512, 1, 8, 3, 3, 2, 3, 'infer', (S_FWD,), NOT_DENSE, gather=True, extra=dict(lds_edge=True)),
    case('gather-fwd-time', 257, 2, 8, 2, 2, 2, 3, 'infer', (S_FWD,), NOT_DENSE + (GT_FWD,), gather=True, tg=True),
    case('gather-bptt-K1-P2-B1', 63, 2, 8, 1, 1, 1, 4, 'train', (S_FWD, S_BWD), NOT_DENSE, gather=True, extra=dict(P=2)),
    case('gather-bptt-K2-P4', 64, 1, 32, 2, 2, 2, 3, 'train', (S_FWD, S_BWD), NOT_DENSE, gather=True, extra=dict(P=4)),
    case('gather-bptt-K3-P2-time', 65, 1, 31, 3, 3, 2, 3, 'train', (S_FWD, S_BWD), NOT_DENSE, gather=True, tg=True, extra=dict(P=2)),
    case('gather-bptt-K4-P4', 69, 2, 30, 4, 4, 2, 3, 'train', (S_FWD, S_BWD), NOT_DENSE, gather=True, extra=dict(P=4)),
    case('gather-bptt-K5-B1-T200-uniform', 33, 3, 16, 5, 5, 1, 200, 'train', (S_FWD, S_BWD), NOT_DENSE, gather=True, uniform=True,
         extra=dict(P=2)),
    # ---- Horner streaming inference (N > 1024: outside the small envelopes)
    case('horner-taps-mfma-spmm-ex', 1100, 16, 16, 3, 3, 2, 3, 'infer', (TAPS_MFMA, SPMM_EX), SMALL + (SPMM, TAPS)),
    case('horner-taps-rows-F20', 1100, 3, 20, 3, 2, 2, 3, 'infer', (TAPS, SPMM_EX), SMALL + (SPMM, TAPS_MFMA)),
    case('horner-scalar-spmm-odd-L', 1100, 2, 21, 3, 3, 3, 3, 'infer', (TAPS, SPMM), SMALL + (SPMM_EX, TAPS_MFMA)),
    case('horner-K1', 1100, 16, 16, 1, 1, 2, 3, 'infer', (TAPS_MFMA,), SMALL + (SPMM, SPMM_EX)),
    case('horner-time', 1100, 3, 16, 2, 2, 2, 3, 'infer', (TAPS, SPMM_EX), SMALL + (TAPS_MFMA,), tg=True),
    case('horner-uniform', 1100, 16, 16, 2, 2, 2, 3, 'infer', (TAPS_MFMA, SPMM_EX), SMALL, uniform=True, f32=False),
    # ---- composed LSIGF with gradients (X wants a gradient, or N > 1024)
    case('composed-E2-F63-parts', 101, 3, 63, 2, 2, 3, 3, 'trainx', (TAPS, TBD, TBW), SMALL, E=2, extra=dict(parts=(909, 2, 3, 63))),
    case('composed-N1030-K7-KG63-F64', 1030, 9, 64, 7, 1, 1, 2, 'train', (TAPS, TBD, TBW), SMALL),
    case('composed-K7-KG70-F65', 77, 10, 65, 7, 7, 2, 2, 'trainx', (TAPS, TBD, TBW), SMALL),
    case('composed-E2-K1-time', 90, 5, 64, 1, 1, 3, 3, 'trainx', (TAPS, TBD, TBW), SMALL + (SPMM, SPMM_EX), E=2, tg=True),
    case('composed-N1030-uniform', 1030, 4, 16, 3, 3, 2, 2, 'trainx', (TAPS, TBD, TBW), SMALL, uniform=True),
    # ---- edge-gated cells around the attention kernels
    case('edge-small-N40', 40, 3, 6, 2, 2, 2, 3, 'trainx', (ATT_F, ATT_B, TAPS), SMALL, sg='edge'),
    case('edge-time-N300', 300, 2, 8, 2, 2, 2, 3, 'train', (ATT_F, ATT_B, TAPS), SMALL, sg='edge', tg=True),
    case('edge-time-N300-uniform-infer', 300, 2, 8, 2, 2, 2, 3, 'infer', (ATT_F, TAPS), SMALL, sg='edge', tg=True, uniform=True),
]


def _init(cell, G, F, Ki, Ks, E):
    """Taps at 1/sqrt(fan-in) (a contracting recurrence: fp32 noise is not amplified over T = 200 steps); read-outs of the time gates and the
    node gates' filters scaled up so that the gates are far from 0.5 (as the G12 / G13 fixtures do)."""
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


def _close(got, ref, tol, what):
    scale = float(ref.abs().max()) + 1e-30
    err = float((got.double() - ref).abs().max())
    assert err <= tol * scale, '%s: %.3g of %.3g' % (what, err, scale)
    return err / scale


def _abs_close(got, ref, tol, what):
    err = float((got.double() - ref).abs().max())
    assert err <= tol, '%s: %.3g' % (what, err)
    return err


@pytest.mark.parametrize('c', CASES)
def test_cell_path_against_torch_reference(c, dev, spy, monkeypatch):
    N, G, F, Ki, Ks, B, T, E = c['N'], c['G'], c['F'], c['Ki'], c['Ks'], c['B'], c['T'], c['E']
    if c['gather']:
        monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')
    else:
        monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    S = graph(N, 1000 + N + 7 * F, c['uniform'], E)
    torch.manual_seed(N + F)
    cell = gml().GGCRNNCell(G, F, Ki, Ks, torch.tanh, c['tg'], c['sg'], E, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.double()
    _init(cell, G, F, Ki, Ks, E)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(B, T, G, N, generator=gen, dtype=torch.float64).to(dev)
    h0 = (0.5 * torch.randn(B, F, N, generator=gen, dtype=torch.float64)).to(dev)
    R = torch.randn(B, T, F, N, generator=gen, dtype=torch.float64).to(dev)
    mode = c['mode']

    # the reference: dense S, fp64, autograd
    Sd = torch.tensor(S, device=dev)
    rp = {k: v.detach().to(dev).clone().requires_grad_(mode != 'infer') for k, v in cell.state_dict().items()}
    Xr, h0r = X.clone().requires_grad_(mode == 'trainx'), h0.clone().requires_grad_(mode != 'infer')
    Hr = tr.ggcrnn_cell(rp, Sd, Xr, h0r, c['tg'], c['sg'])
    if mode != 'infer':
        (Hr * R).sum().backward()

    ex = c['extra']
    if 'parts' in ex:          # the weight-gradient GEMM splits its row reduction: T N B rows not a multiple of 16, more than one split
        rows, KK, GG, FF = ex['parts']
        assert rows == T * N * B and rows % 16
        nsp, nbb = C.c_int64(0), C.c_int64(0)
        assert ops().lib.gcrnn_taps_backward_weight_parts(rows, KK, GG, FF, C.byref(nsp), C.byref(nbb)) == 0
        assert nsp.value > 1 and nbb.value > 1, (nsp.value, nbb.value)
    if 'lds_edge' in ex:       # the largest fp64 gather shape: one more tap does not fit 150 KB of LDS
        nnz = int(np.count_nonzero(S[0]))
        assert ops().small_supported(N, nnz, G, F, Ki, Ks, torch.float64)
        assert not ops().small_supported(N, nnz, G, F, Ki + 1, Ks + 1, torch.float64)
    if 'P' in ex:              # the backward kernel's slot passes: P = 2 iff F N <= 2048 and 2 F (G + F) <= 2048
        assert (2 if (F * N <= 2048 and 2 * F * (G + F) <= 2048) else 4) == ex['P']
    if 'tiles' in ex:
        assert ((N + 15) // 16) * ((F + 15) // 16) == ex['tiles']
    if 'wtiles' in ex:
        assert max(Ki, Ks) * ((F + 15) // 16) * ((G + F + 15) // 16) == ex['wtiles']
    if 'gate_tiles' in ex:
        assert ((F + 15) // 16) * ((Ki * ((G + 3) // 4 * 4) + 15) // 16) == ex['gate_tiles']

    for dt in (torch.float64, torch.float32):
        stol, gtol = TOLS[dt]
        cd = copy.deepcopy(cell).to(dev).to(dt)
        Xd = X.to(dt).clone().requires_grad_(mode == 'trainx')
        h0d = h0.to(dt).clone().requires_grad_(mode != 'infer')
        spy.calls.clear()
        if mode == 'infer':
            with torch.no_grad():
                H = cd(Xd, h0d)
        else:
            H = cd(Xd, h0d)
            (H * R.to(dt)).sum().backward()
        torch.cuda.synchronize()
        if dt == torch.float64 or c['f32']:
            ran = set(spy.calls)
            for name in c['runs']:
                assert name in ran, '%s: %s did not run (ran: %s)' % (dt, name, sorted(ran))
            for name in c['not_runs']:
                assert name not in ran, '%s: %s ran (ran: %s)' % (dt, name, sorted(ran))
        assert H.dtype == dt and tuple(H.shape) == (B, T, F, N)
        _abs_close(H.detach(), Hr.detach(), stol, '%s states' % dt)
        if mode == 'infer':
            continue
        got = dict(cd.named_parameters())
        for k, v in rp.items():
            if v.grad is None or float(v.grad.abs().max()) == 0.0:
                assert got[k].grad is None or float(got[k].grad.abs().max()) == 0.0, k
                continue
            assert got[k].grad is not None, '%s: no gradient for %s' % (dt, k)
            _close(got[k].grad, v.grad, gtol, '%s grad %s' % (dt, k))
        _close(h0d.grad, h0r.grad, gtol, '%s grad h0' % dt)
        if mode == 'trainx':
            _close(Xd.grad, Xr.grad, gtol, '%s grad X' % dt)


GFL_CASES = [
    pytest.param(dict(N=37, Fin=5, Fout=5, K=1, items=3, uniform=False), id='K1-Fout=Fin-hops-first-VEC1'),
    pytest.param(dict(N=64, Fin=4, Fout=1, K=7, items=3, uniform=False), id='KO7-taps-first-VEC4'),
    pytest.param(dict(N=50, Fin=3, Fout=2, K=4, items=4, uniform=True), id='KO8-uniform-VEC1'),
    pytest.param(dict(N=100, Fin=8, Fout=3, K=3, items=2, uniform=False), id='KO9-VEC4'),
    pytest.param(dict(N=1000, Fin=8, Fout=8, K=2, items=None, uniform=True), id='items>wgrad_slots-uniform'),
    pytest.param(dict(N=1000, Fin=4, Fout=5, K=2, items=None, uniform=False), id='items>wgrad_slots-weighted'),
]


@pytest.mark.parametrize('c', GFL_CASES)
def test_graph_filter_layer_against_torch_reference(c, dev, spy, monkeypatch):
    """ops.graph_filter_layer on gcrnn_graph_filter_layer_{forward,backward} (the composed fallback made to raise) for every activation."""
    from gated_gcrnns_amd.graph import GraphOperator
    N, Fin, Fout, K = c['N'], c['Fin'], c['Fout'], c['K']

    def no_fallback(*a, **k):
        raise AssertionError('composed fallback taken')
    monkeypatch.setattr(ops(), '_graph_filter_layer_composed', no_fallback)
    S = graph(N, 2000 + N + Fout, c['uniform'])
    g = GraphOperator(S, device=dev)
    assert (ops()._gfl_uniform(g.fwd[0]) != 0.0) == c['uniform']
    items = c['items']
    if items is None:          # more items than weight-gradient slots: slots are reused
        code, uni = ops().dtype_code(torch.float64), int(c['uniform'])
        cap = int(ops().lib.gcrnn_graph_filter_layer_wgrad_slots(code, 1 << 40, N, g.adj[0].nnz, Fin, Fout, K, uni))
        assert 0 < cap <= 1024
        items = cap + 37
    gen = torch.Generator().manual_seed(N + K)
    x = torch.randn(items, Fin, N, generator=gen, dtype=torch.float64).to(dev)
    w = (torch.rand(Fout, 1, K, Fin, generator=gen, dtype=torch.float64) * 2 - 1).to(dev) / np.sqrt(Fin * K)
    b = (torch.rand(Fout, 1, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    R = torch.randn(items, Fout, N, generator=gen, dtype=torch.float64).to(dev)
    Sd = torch.tensor(S, device=dev)
    for act in (None, 'relu', 'tanh', 'sigmoid'):
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yr = tr.graph_filter_layer(wr, br, Sd, xr, act)
        (yr * R).sum().backward()
        for dt in (torch.float64, torch.float32):
            stol, gtol = TOLS[dt]
            assert ops().graph_filter_layer_supported(dt, dt, g, Fin, Fout, K)
            xd, wd, bd = (t.to(dt).clone().requires_grad_(True) for t in (x, w, b))
            spy.calls.clear()
            y = ops().graph_filter_layer(xd, wd, bd, g, act)
            (y * R.to(dt)).sum().backward()
            torch.cuda.synchronize()
            assert spy.calls[GFL_F] == 1 and spy.calls[GFL_B] == 1, dict(spy.calls)
            _close(y.detach(), yr.detach(), stol, '%s %s y' % (dt, act))
            _close(xd.grad, xr.grad, gtol, '%s %s dx' % (dt, act))
            _close(wd.grad, wr.grad, gtol, '%s %s dw' % (dt, act))
            _close(bd.grad, br.grad, gtol, '%s %s db' % (dt, act))
