"""GPU (-m gpu): the own parameter gradients of the heads inside the small-graph launches (ops._node_head_grads / _readout_grads, through
the public entries small_cell_regress, small_cell_regress_gnn, small_cell_classify_gnn and small_edge_cell_regress) against an fp64 einsum
on the same stored states -- with torch.equal, because every expected sum is exact:

  states    X is 32 x (an odd integer), the k = 0 input taps are odd integers, every other tap and the bias contribute an even multiple of
            32 (a column of S holds two ones, a state is +-1), so every pre-activation is an odd multiple of 32 and tanh gives +-1 exactly
            in fp64 (the edge-gated cell: 0 or 1, its gates end in a ReLU). The test asserts that on the states the cell's own forward
            stores.
  upstream  the loss is sum(Y . W) with W small multiples of 1/8, the head has no activation and S is 0 / 1, so dY, and the graph-filter
            heads' adjoint levels dU_k = dU_{k-1} S^T, are small multiples of 1/64 whatever the order they are summed in.
  expected  d w[o][f] = sum_{r,n} dU[r][o][n] H[r][f][n]: at most B T N = 45 terms of magnitude <= 4 on a grid of 1/64 -- exact in any order.

F = 4 takes node_linear's slot kernel, F = 68 (node_linear_supported ends at 64) the batched product; O / K_o in {1, 3}; with and without a
head bias; weight and bias asking for a gradient together and one at a time. A counting wrapper shows when the slot kernel ran: the
per-node heads run it only for the weight, the graph-filter heads for either."""
import functools

import pytest
import torch

from test_small_head import _CountingLib

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F64 = torch.float64
N, G, K, B, T, C = 5, 1, 2, 3, 3, 3
NL_BWD = 'gcrnn_node_linear_backward'
#         head bias, weight wants a gradient, bias wants one
WANTS = [(True, True, True), (True, True, False), (True, False, True), (False, True, False)]
WANT_IDS = ['w+b', 'w', 'b', 'nobias']


def ops():
    from gated_gcrnns_amd import ops as m
    return m


@pytest.fixture
def spy(monkeypatch):
    o = ops()
    s = _CountingLib(o.lib)
    monkeypatch.setattr(o, 'lib', s)
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    return s


def _ring():
    """Directed 0 / 1 GSO: node m feeds m + 1 and m + 2, so every row and every column holds two ones."""
    S = torch.zeros(N, N, dtype=F64)
    for m in range(N):
        S[m, (m + 1) % N] = S[m, (m + 2) % N] = 1.0
    assert not torch.equal(S, S.t())
    return S


@functools.lru_cache(maxsize=None)
def _cell(F, edge):
    """Seeded operands of the cell (shared, never written) and the states its own forward stores, all +-1 (edge-gated: 0 or 1)."""
    from gated_gcrnns_amd.graph import GraphOperator
    gen = torch.Generator().manual_seed(7 * F + edge)

    def ints(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=gen).double()

    def odd(lo, hi, *s):                                   # odd integers in [2 lo + 1, 2 hi + 1]
        return 2 * ints(lo, hi, *s) + 1
    c = dict(graph=GraphOperator(_ring()[None], device=DEV), S=_ring().to(DEV))
    wA = torch.stack((odd(-2, 1, F, G), ints(-3, 3, F, G)), dim=1).unsqueeze(1)             # [F][1][Kin][G]: k = 0 odd
    t = dict(X=32 * odd(-4, 3, B, T, G, N), h0=odd(-1, 0, B, F, N), wA=wA, wB=64 * ints(-1, 1, F, 1, K, F), b=32 * ints(-1, 1, F, 1))
    if edge:       # (S + I) . attention with a zero mixer averages three neighbours, then a ReLU: input branch 32 x odd or 0, state branch 0
        t['X'], t['wB'], t['b'] = 3 * t['X'], torch.zeros_like(t['wB']), None
        t.update(m_in=torch.zeros(1, 1, 2 * F, dtype=F64), w_in=torch.eye(F, dtype=F64).reshape(1, 1, F, F),
                 m_f=torch.zeros(1, 1, 2 * F, dtype=F64), w_f=torch.eye(F, dtype=F64).reshape(1, 1, F, F))
    c.update({k: v.to(DEV) if v is not None else None for k, v in t.items()})
    o = ops()
    # fail, not skip: the shapes were chosen inside the matrix-core family's envelope (K tilesF tilesC = 2 * 5 * 5 <= 64 at F = 68)
    assert edge or o.small_dense_supported(N, G, F, K, K, F64, backward=True, gated=False), F
    assert o.node_linear_supported(F, 3, F64) == (F <= 64)
    with torch.no_grad():
        if edge:
            H = o.small_edge_cell_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'], (c['m_in'], c['w_in']), (c['m_f'], c['w_f']))
        else:
            H = o.small_cell_forward(c['X'], c['h0'], c['wA'], c['wB'], c['b'], c['graph'])
    other = 0 if edge else -1                              # (an edge gate ends in a ReLU: its states are 0 or 1)
    assert tuple(H.shape) == (B, T, F, N) and bool(((H == 1) | (H == other)).all()), 'the states are not saturated: the sums below would not be exact'
    assert 0 < int((H == 1).sum()) < H.numel()
    c['H'] = H
    return c


def _eighths(gen, lo, hi, *s):
    """Multiples of 1/8 in [lo, hi], none zero."""
    v = torch.randint(int(8 * lo), int(8 * hi) + 1, s, generator=gen).double()
    return (torch.where(v == 0, torch.ones_like(v), v) / 8).to(DEV)


def _levels(dU0, S, Ko):
    """dU_0 .. dU_{K_o - 1} stacked before the node axis, dU_k = dU_{k-1} S^T (exact: S is 0 / 1)."""
    lv = [dU0]
    for _ in range(1, Ko):
        lv.append(lv[-1] @ S.t())
    return torch.stack(lv, dim=-2)


def _check(got, expected, name):
    assert got is not None, name
    assert got.dtype == expected.dtype and tuple(got.shape) == tuple(expected.shape), (name, got.shape, expected.shape)
    print('%s: max |got - expected| = %g' % (name, float((got - expected).abs().max())))
    assert torch.equal(got, expected), name


def _head(gen, O, F, bias, want_w, want_b):
    w = _eighths(gen, -1, 1, O, F).requires_grad_(want_w)
    return w, (_eighths(gen, -1, 1, O).requires_grad_(want_b) if bias else None)


def _kernel_ran(spy, F, yes):
    assert spy.calls[NL_BWD] == (1 if yes and F <= 64 else 0), dict(spy.calls)


def cases(fn):
    fn = pytest.mark.parametrize('bias,want_w,want_b', WANTS, ids=WANT_IDS)(fn)
    return pytest.mark.parametrize('O', [1, 3])(fn)


@cases
@pytest.mark.parametrize('F,edge', [(4, False), (68, False), (4, True)], ids=['F4', 'F68', 'edge-F4'])
def test_per_node_head(spy, F, edge, O, bias, want_w, want_b):
    """small_cell_regress and small_edge_cell_regress: d node_w and all O bias sums; the slot kernel runs only for the weight."""
    c, o = _cell(F, edge), ops()
    gen = torch.Generator().manual_seed(100 * F + 10 * O + 2 * want_w + want_b)
    w, b = _head(gen, O, F, bias, want_w, want_b)
    W = _eighths(gen, -1, 1, B, T, O, N)
    wA = c['wA'].clone().requires_grad_(True)              # the cell always trains: the node runs also where one head gradient is off
    if edge:
        Y = o.small_edge_cell_regress(c['X'], c['h0'], wA, c['wB'], c['b'], c['graph'], (c['m_in'], c['w_in']), (c['m_f'], c['w_f']), w, b)
    else:
        Y = o.small_cell_regress(c['X'], c['h0'], wA, c['wB'], c['b'], c['graph'], w, b)
    (Y * W).sum().backward()
    _kernel_ran(spy, F, want_w)
    assert wA.grad is not None and bool(torch.isfinite(wA.grad).all())
    if want_w:
        _check(w.grad, torch.einsum('btfn,bton->of', c['H'], W), 'd node_w')
    else:
        assert w.grad is None
    if want_b:
        _check(b.grad, W.sum(dim=(0, 1, 3)), 'd node_b')
    else:
        assert b is None or b.grad is None


@cases
@pytest.mark.parametrize('F', [4, 68])
def test_graph_filter_head(spy, F, O, bias, want_w, want_b):
    """small_cell_regress_gnn (K_o = O taps, no activation): d head_w over every state and level 0's sum as the [1] bias gradient; the
    slot kernel runs for either."""
    c, o = _cell(F, False), ops()
    gen = torch.Generator().manual_seed(200 * F + 10 * O + 2 * want_w + want_b)
    w, b = _head(gen, O, F, bias, want_w, want_b)
    b = b[:1].detach().requires_grad_(want_b) if bias else None
    W = _eighths(gen, -1, 1, B, T, 1, N)
    wA = c['wA'].clone().requires_grad_(True)
    Y = o.small_cell_regress_gnn(c['X'], c['h0'], wA, c['wB'], c['b'], c['graph'], w, b, None)
    (Y * W).sum().backward()
    _kernel_ran(spy, F, want_w or want_b)
    dU = _levels(W[:, :, 0], c['S'], O)                    # [B][T][K_o][N]
    if want_w:
        _check(w.grad, torch.einsum('btfn,btkn->kf', c['H'], dU), 'd head_w')
    else:
        assert w.grad is None
    if want_b:
        _check(b.grad, dU[:, :, 0].sum().view(1), 'd head_b')
    else:
        assert b is None or b.grad is None


@cases
@pytest.mark.parametrize('F', [4, 68])
def test_graph_filter_head_and_read_out(spy, F, O, bias, want_w, want_b):
    """small_cell_classify_gnn (K_o = O taps, no activation, C classes): d head_w over the B last states, level 0's sum, and the read-out's
    own d lin_w = dlogits^T V, d lin_b."""
    c, o = _cell(F, False), ops()
    gen = torch.Generator().manual_seed(300 * F + 10 * O + 2 * want_w + want_b)
    w, b = _head(gen, O, F, bias, want_w, want_b)
    b = b[:1].detach().requires_grad_(want_b) if bias else None
    lw, lb = _eighths(gen, -1, 1, C, N).requires_grad_(True), _eighths(gen, -1, 1, C).requires_grad_(True)
    W = _eighths(gen, -1, 1, B, C)
    wA = c['wA'].clone().requires_grad_(True)
    logits = o.small_cell_classify_gnn(c['X'], c['h0'], wA, c['wB'], c['b'], c['graph'], w, b, lw, lb, None)
    (logits * W).sum().backward()
    _kernel_ran(spy, F, want_w or want_b)
    hT, S = c['H'][:, -1], c['S']
    dU = _levels(W @ lw.detach(), S, O)                    # [B][K_o][N]
    if want_w:
        _check(w.grad, torch.einsum('bfn,bkn->kf', hT, dU), 'd head_w')
    else:
        assert w.grad is None
    if want_b:
        _check(b.grad, dU[:, 0].sum().view(1), 'd head_b')
    else:
        assert b is None or b.grad is None
    Z = [hT]                                               # V = sum_k w_k (h_T S^k) + b: integers / 8
    for _ in range(1, O):
        Z.append(Z[-1] @ S)
    V = torch.einsum('kf,bkfn->bn', w.detach(), torch.stack(Z, dim=1)) + (b.detach() if bias else 0)
    _check(lw.grad, W.t() @ V, 'd lin_w')
    _check(lb.grad, W.sum(dim=0), 'd lin_b')
