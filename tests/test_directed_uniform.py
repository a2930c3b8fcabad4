"""The uniform-weight and rank-1 kernels on DIRECTED graphs.

tests/test_wide.py, tests/test_wide_head.py and the uniform / x3 / rank-1 tests of tests/test_fused.py build every graph as
W = triu(W, 1); W + W.T: on a symmetric support the forward plan (CSR(S^T)) and the adjoint plan (CSR(S)) are the same object in the
same degree order, so a launch given the wrong plan, swapped rank-1 factors, a permutation shared between two plans or S @ x in place of
the reference's x @ S all go unseen. Here the same kernels run on directed 0/1 graphs (uniform weight) and on their normalisations
(rank-1 weights), against the fp64 oracle (oracle/gcrnn_oracle.py) for the states and the plain-torch fp64 restatement under autograd
(oracle/torch_reference.py, tied to the reference's own autograd by tests/test_torch_reference.py) for the gradients. Every case first
proves on the CPU, from the reference alone, that it can fail on a transposition: max |ref(S) - ref(S^T)| >= 20 x its tolerance.

Tolerances are those of the symmetric-graph test of the same kernel; the graphs are scaled by their largest SINGULAR value (a directed A
is not normal: with ||S||_2 = 1 the growth per hop is what |lambda|max = ||S||_2 gives the symmetric tests). Where a transposed graph
moves a reference by less than 20 of the symmetric test's tolerances, the bound here is TIGHTER (node- and edge-gated H 1.2e-2, the
gradients that see the direction 1.5e-2, filter output 2e-2, d h0 of the chain 1.5e-2, dW tap by tap, dpre elementwise: DPRE_TOL), never
wider.

Measured on an MI355X (GCRNN_TOL_REPORT; worst case of each group next to its bound):
  bf16 forward |H - oracle|: wide / hand-allocated hop 3.2e-3 max, 4.8e-4 mean; 16-feature / step 2.6e-3, 4.5e-4 (5e-3 / 1e-3; time-gated
    2.4e-3 against 6e-3); G = 1: 3.0e-2 (6e-2); head 3.9e-3 (||w||_1 x 5e-3 = 1.8e-2); node-gated 3.3e-3, edge-gated 2.7e-3 (1.2e-2)
  bf16 training, of each gradient's max: d X 6.9e-3, d h0 5.0e-3, weight_B 2.6e-3 (1.5e-2); every other parameter <= 1.8e-2 (5e-2);
    rank-1 graphs: d X 7.2e-3, others <= 1.6e-2; H 3.2e-3 (8e-3). Edge-gated training: see EDGE_KNOWN_MISSES
  ops level: filter output 2.7e-3 (2e-2); dpre 0.62 of its elementwise bound; d h0 4.1e-3 (1.5e-2); dW taps 2.6e-3 (2e-2)
  x3: H 4.7e-7 uniform, 5.5e-7 rank-1 (1e-5); gradients 1.4e-6 of their max (2e-5)
  rank-1 wide forward 3.2e-3 max, 4.7e-4 mean (5e-3 / 1e-3)
No bound had to be set from the bf16-state emulation."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from oracle import torch_reference as tref
from test_fused import _grad_scale_and_bounds, _tol_report

GRAPH_SEED = 7
SMALL = (400, 32, 32, 3)          # (N, F, G, K): one 32-feature chunk per step, no state scratch
LARGE = (1000, 64, 64, 5)         # two chunks per step, state scratch
ONE_IN = (1000, 64, 1, 3)         # the drivers' single input feature, padded to 32 channels (forward only)
MARGIN = 20.0                     # a transposed graph must move the reference by this many tolerances


# ------------------------------------------------------------------------------------------------------------ graphs (numpy only)
def special_nodes(N):
    """The nodes with a prescribed role, spread over the id range (distinct for N >= 64)."""
    ids = [1 + i * (N // 16) for i in range(14)]
    return dict(no_in=ids[0:4], no_out=ids[4:8], isolated=ids[8:10], loops=ids[10:12], hub=ids[12], hub_to=ids[13])


@functools.lru_cache(maxsize=None)
def directed_pattern(N, seed):
    """0/1 matrix of density 10 / N, NOT symmetrised (A[m][n] = 1: the reference's x @ S carries node m's signal to node n), with
    4 nodes nobody sends to (empty column, non-empty row), 4 nodes that send to nobody (empty row, non-empty column), 2 isolated nodes,
    exactly 2 self-loops, and a hub that about N / 8 nodes send to and that sends to exactly one: first in the forward degree order,
    last among the connected nodes in the adjoint one."""
    rng = np.random.default_rng(seed)
    A = (rng.random((N, N)) < 10.0 / N).astype(np.float64)
    np.fill_diagonal(A, 0.0)
    r = special_nodes(N)
    taken = set(r['no_in']) | set(r['no_out']) | set(r['isolated']) | {r['hub'], r['hub_to']}
    plain = np.array([n for n in range(N) if n not in taken])
    for n in r['no_in'] + r['isolated'] + [r['hub']]:
        A[:, n] = 0.0
    for n in r['no_out'] + r['isolated'] + [r['hub']]:
        A[n, :] = 0.0
    for i, n in enumerate(r['no_in']):
        A[n, plain[(7 * i + 3) % plain.size]] = 1.0
    for i, n in enumerate(r['no_out']):
        A[plain[(11 * i + 5) % plain.size], n] = 1.0
    for n in r['loops']:
        A[n, n] = 1.0
    A[rng.choice(plain, N // 8, replace=False), r['hub']] = 1.0
    A[r['hub'], r['hub_to']] = 1.0
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def directed_uniform(N, seed):
    """The pattern divided by its largest singular value: 1 x N x N, fp64, one weight on every edge."""
    A = directed_pattern(N, seed)
    S = (A / np.linalg.norm(A, 2)).reshape(1, N, N)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def directed_rank1(N, seed, kind):
    """'out': D_out^-1 A, 'in': A D_in^-1, 'sym': D_out^-1/2 A D_in^-1/2 of the same pattern (zero degrees count as 1), divided by the
    largest singular value: S[m][n] = a[m] b[n] on the support, fp64."""
    A = directed_pattern(N, seed)
    dout = A.sum(axis=1); dout[dout == 0] = 1.0
    din = A.sum(axis=0); din[din == 0] = 1.0
    if kind == 'out':
        S = A / dout[:, None]
    elif kind == 'in':
        S = A / din[None, :]
    else:
        assert kind == 'sym'
        S = A / np.sqrt(dout)[:, None] / np.sqrt(din)[None, :]
    S = (S / np.linalg.norm(S, 2)).reshape(1, N, N)
    S.setflags(write=False)
    return S


def _gso(kind, N):
    return directed_uniform(N, GRAPH_SEED) if kind == 'uni' else directed_rank1(N, GRAPH_SEED, kind)


@functools.lru_cache(maxsize=None)
def _cpu_graph(kind, N):
    """One host-side GraphOperator per graph, shared by the CPU cases (its plans are cached on it and never written to)."""
    from gated_gcrnns_amd.graph import GraphOperator
    return GraphOperator(_gso(kind, N))


def _assert_structure(N):
    """The builder delivers what the cases rely on."""
    A, r = directed_pattern(N, GRAPH_SEED), special_nodes(N)
    rows, cols = A.sum(axis=1), A.sum(axis=0)
    assert len({n for v in r.values() for n in (v if isinstance(v, list) else [v])}) == 14
    assert not np.array_equal(A, A.T)
    assert all(cols[n] == 0 and rows[n] > 0 for n in r['no_in']) and all(rows[n] == 0 and cols[n] > 0 for n in r['no_out'])
    assert all(rows[n] == 0 and cols[n] == 0 for n in r['isolated'])
    assert int(np.trace(A)) == 2 and all(A[n, n] == 1 for n in r['loops'])
    assert cols[r['hub']] == N // 8 and rows[r['hub']] == 1 and cols[r['hub']] == cols.max()


def _assert_directed(graph, S):
    """CPU, before any launch: the support is not symmetric and the two plans do not share a degree order."""
    assert not np.array_equal(S[0] != 0, S[0].T != 0)
    assert not torch.equal(graph.fused_plan()['order'], graph.fused_plan(adjoint=True)['order'])


def _assert_rank1(graph, S):
    """rank1_factors finds the graph, and each factor table has zeros at nodes where the other one has none."""
    f = graph.rank1_factors()
    assert f is not None, 'rank1_factors() did not find an exactly rank-1 directed graph'
    a, b = f
    assert np.any((a == 0) & (b != 0)) and np.any((b == 0) & (a != 0))
    assert graph.fused_plan()['uniform_w'] == 0.0
    return f


# ------------------------------------------------------------------------------------------------------------ problems and references
def bf16_round(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(torch.bfloat16).double().numpy()


def f32_round(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _new_cell(G, F, K, tg, sg, S):
    import gated_gcrnns_amd.Utils.graphML as gml
    cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, tg, sg, 1, True)
    cell.addGSO(torch.tensor(np.asarray(S)))
    return cell


@functools.lru_cache(maxsize=None)
def _problem(kind, shape, B, T, tg=False, sg=None, prec='bf16'):
    """One problem and its fp64 references, computed once and shared (never written to): operands and parameters rounded to the
    precision the kernels read (bf16, or fp32 for the x3 kernels), the oracle on S rounded to fp32 -- and on its TRANSPOSE, for the
    discrimination condition."""
    N, F, G, K = shape
    S = _gso(kind, N)
    rnd = bf16_round if prec == 'bf16' else f32_round
    seed = 211 + N + 7 * K + (1 if tg else 0) + {None: 0, 'node': 2, 'edge': 4}[sg]
    torch.manual_seed(seed)
    cell = _new_cell(G, F, K, tg, sg, S)
    with torch.no_grad():
        if tg:                                          # make the scalar gates vary, as the symmetric tests do
            scale = 8.0 if prec == 'bf16' else 6.0
            cell.MLP_in[0].weight.mul_(scale)
            cell.MLP_forget[0].weight.mul_(scale)
    state = {k: torch.tensor(rnd(v.detach().float().numpy()), dtype=torch.float32) for k, v in cell.state_dict().items()}
    params = {k: v.double().numpy() for k, v in state.items()}
    rng = np.random.default_rng(seed)
    X = rnd(rng.standard_normal((B, T, G, N)))
    h0 = rnd(0.3 * rng.standard_normal((B, F, N)))
    dH = rnd(rng.standard_normal((B, T, F, N)))
    S32 = f32_round(S)
    H = orc.ggcrnn_cell(params, S32, X, h0, tg, sg)
    Ht = orc.ggcrnn_cell(params, np.ascontiguousarray(S32.transpose(0, 2, 1)), X, h0, tg, sg)
    for a in (X, h0, dH, H, Ht):
        a.setflags(write=False)
    return types.SimpleNamespace(kind=kind, shape=shape, N=N, F=F, G=G, K=K, B=B, T=T, tg=tg, sg=sg, prec=prec, S=S, S32=S32, state=state,
                                 params=params, X=X, h0=h0, dH=dH, H=H, Ht=Ht, graph=cell.graph)


def _torch_grads(p, S32):
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.params.items()}
    X = torch.tensor(p.X, dtype=torch.float64, requires_grad=True)
    h0 = torch.tensor(p.h0, dtype=torch.float64, requires_grad=True)
    H = tref.ggcrnn_cell(P, torch.tensor(S32, dtype=torch.float64), X, h0, p.tg, p.sg)
    (H * torch.tensor(p.dH, dtype=torch.float64)).sum().backward()
    g = {k: v.grad.numpy() for k, v in P.items() if v.grad is not None and float(v.grad.abs().max()) > 0}
    g['dX'], g['dh0'] = X.grad.numpy(), h0.grad.numpy()
    return g


@functools.lru_cache(maxsize=None)
def _grads(kind, shape, B, T, tg=False, sg=None, prec='bf16'):
    """Reference gradients of loss = (H * dH).sum() under torch autograd in fp64 on the CPU, for S and for its transpose."""
    p = _problem(kind, shape, B, T, tg, sg, prec)
    return _torch_grads(p, p.S32), _torch_grads(p, np.ascontiguousarray(p.S32.transpose(0, 2, 1)))


def _assert_discriminates(p, tol, what='H', ref=None, reft=None):
    ref, reft = (p.H, p.Ht) if ref is None else (ref, reft)
    d = float(np.abs(ref - reft).max())
    assert d >= MARGIN * tol, 'a transposed graph moves %s by %.3g only: %.1f x the tolerance %.3g' % (what, d, d / tol, tol)


def _assert_grads_discriminate(g, gt, keys, tol):
    for k in keys:
        sc = float(np.abs(g[k]).max())
        d = float(np.abs(g[k] - gt[k]).max())
        assert d >= MARGIN * tol * sc, 'a transposed graph moves the gradient %s by %.3g of its max only (tolerance %.3g)' % (k, d / sc, tol)


def _device_cell(p, dtype):
    cell = _new_cell(p.G, p.F, p.K, p.tg, p.sg, p.S)
    cell.load_state_dict(p.state)
    return cell.float().to(torch.device('cuda:0')).to(dtype)


def _operands(p, dtype, n=None):
    dev = torch.device('cuda:0')
    return torch.tensor(p.X[:n], dtype=dtype, device=dev), torch.tensor(p.h0[:n], dtype=dtype, device=dev)


FORWARD_ENV = {'wide': {'GCRNN_SEQ32_MIN_B': '1', 'GCRNN_SEQ32P': '0'},
               'hop': {'GCRNN_SEQ32_MIN_B': '1', 'GCRNN_SEQ32P': '1'},
               'seq16': {'GCRNN_SEQ32': '0', 'GCRNN_SEQ_MIN_B': '1'},
               'step': {'GCRNN_SEQ32': '0', 'GCRNN_SEQ_KERNEL': '0'}}


def _setenv(monkeypatch, env):
    for k in ('GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ32P', 'GCRNN_SEQ32', 'GCRNN_SEQ_MIN_B', 'GCRNN_SEQ_KERNEL', 'GCRNN_NO_INLINE_PACK', 'GCRNN_NO_WIDE_CHAIN',
              'GCRNN_SEQ32_NODE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _h_bounds(p):
    """(max, mean) bound on |H - oracle| of the bf16 kernels: those of the symmetric-graph tests (tests/test_wide.py)."""
    if p.sg is not None:
        # (tests/test_fused.py, node- and edge-gated forward. tests/test_wide.py allows the node-gated wide passes 2.5e-2, but the gates
        # halve the pre-activations: a transposed graph moves H by 0.27 .. 0.44 only, under 20 x 2.5e-2)
        return 1.2e-2, 1.5e-3
    if p.G == 1:
        return 6.0e-2, 2.5e-3
    return (6.0e-3 if p.tg else 5.0e-3), 1.0e-3


def _check_h(tag, H, p, mx, mn, n=None):
    err = np.abs(H.detach().double().cpu().numpy() - p.H[:n])
    line = 'directed %s %s N=%d K=%d G=%d tg=%s sg=%s: |H - oracle| max %.3e mean %.3e (bounds %.1e / %.1e)' % (
        tag, p.kind, p.N, p.K, p.G, p.tg, p.sg, err.max(), err.mean(), mx, mn)
    print(line)
    _tol_report(line)
    assert err.max() <= mx and err.mean() <= mn, (tag, err.max(), err.mean())
    return err


# ------------------------------------------------------------------------------------------------------------ h. CPU
@pytest.mark.parametrize('N', [400, 1000])
def test_directed_builders_deliver_the_structure(N):
    """CPU: the roles the cases rely on (empty rows / columns, isolated nodes, self-loops, the hub), a non-symmetric support, the
    uniform-weight plans in both directions with different degree orders and entry counts, ||S||_2 = 1."""
    from gated_gcrnns_amd.graph import GraphOperator
    _assert_structure(N)
    S = directed_uniform(N, GRAPH_SEED)
    assert abs(np.linalg.norm(S[0], 2) - 1.0) <= 1e-12
    g = _cpu_graph('uni', N)
    _assert_directed(g, S)
    pf, pa = g.fused_plan_img16(), g.fused_plan_img16(adjoint=True)
    assert pf is not None and pa is not None and pf['uniform_w'] != 0.0 and pf['uniform_w'] == pa['uniform_w']
    assert pf['entries'] != pa['entries']
    hub = special_nodes(N)['hub']
    assert int(g.fused_plan()['order'][0]) == hub and int(g.fused_plan(adjoint=True)['order'][0]) != hub
    for kind in ('out', 'in', 'sym'):
        R = directed_rank1(N, GRAPH_SEED, kind)
        assert abs(np.linalg.norm(R[0], 2) - 1.0) <= 1e-12 and np.array_equal(R != 0, S != 0)


def _dense_from_img16(plan, N):
    """The 0/1 operator a bf16-image plan encodes: tile slot -> destination node (tile_nodes), and per group of four entries the four
    uint16 image addresses (entry 0, 2, 1, 3) of the gathered rows, mapped back to nodes through node_addr16."""
    npad, ent = plan['npad'], plan['entries']
    addr16 = plan['node_addr16'].cpu().numpy().astype(np.int64)
    assert len(set(addr16.tolist())) == npad                    # one image row per node (padding rows included)
    node_of = np.full(1 << 16, -1, dtype=np.int64)
    node_of[addr16] = np.arange(npad)
    tn = plan['tile_nodes'].cpu().numpy().astype(np.int64)
    assert sorted(tn.tolist()) == list(range(npad))
    ts = plan['tile_slots'].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(ts >> 16, tn) and np.array_equal(ts & 0xFFFF, addr16[tn])
    toff = plan['tile_off'].cpu().numpy().astype(np.int64)
    assert toff[0] == 0 and toff[-1] == ent and np.all(np.diff(toff) % 4 == 0)
    col4 = plan['ell_col4'].cpu().numpy().view(np.uint16).astype(np.int64).reshape(ent // 4, 16, 4)
    tile_of_group = np.repeat(np.arange(npad // 16), np.diff(toff) // 4)                 # [group] -> tile
    dst = np.broadcast_to(tn.reshape(npad // 16, 16)[tile_of_group][:, :, None], col4.shape)   # [group][slot][entry] -> destination node
    src = node_of[col4]
    assert src.min() >= 0                                       # every address is some node's image row
    P = np.zeros((npad, npad))
    np.add.at(P, (dst.reshape(-1), src.reshape(-1)), 1.0)
    assert not P[N:, :N].any()                                  # padding rows gather nothing real
    return P[:N, :N]                                            # (columns >= N: padding entries aimed at the all-zero padding rows)


@pytest.mark.parametrize('N', [400, 1000])
def test_bf16_image_plans_reproduce_the_directed_pattern(N):
    """CPU: the dense operator rebuilt from fused_plan_img16() is the pattern of S^T (the forward shift x @ S gathers, for node n, the
    rows m with S[m][n] != 0) and from fused_plan_img16(adjoint=True) that of S -- not the other way round, which a symmetric graph
    cannot tell (test_ell_plan_reproduces_shift_exactly does this for the fp32 ELL on weighted graphs)."""
    from gated_gcrnns_amd.graph import GraphOperator
    S = directed_uniform(N, GRAPH_SEED)
    g = _cpu_graph('uni', N)
    _assert_directed(g, S)
    pat = (S[0] != 0).astype(np.float64)
    fwd = _dense_from_img16(g.fused_plan_img16(), N)
    adj = _dense_from_img16(g.fused_plan_img16(adjoint=True), N)
    assert np.array_equal(fwd, pat.T) and np.array_equal(adj, pat)
    assert not np.array_equal(fwd, adj)
    w = np.float32(S[0][S[0] != 0][0])
    assert g.fused_plan_img16()['uniform_w'] == float(w) and g.fused_plan_img16(adjoint=True)['uniform_w'] == float(w)


@pytest.mark.parametrize('kind', ['out', 'in', 'sym'])
@pytest.mark.parametrize('N', [400, 1000])
def test_rank1_factors_of_directed_graphs_are_found_exact_and_swap_with_the_direction(N, kind):
    """CPU: the three normalisations of a directed 0/1 pattern are exactly rank-1 on the support and must be FOUND, given in fp64 (at
    N = 1000 the hub's column averages 125 quotients: a plain mean lost the 8-eps verification to its own rounding and the graph ran the
    slower weighted path): outer(a, b) * pattern == S to 1e-12, the adjoint factors are the swap, both tables have zeros where the other
    has none, and the rank-1 plans of both directions are the pattern's plans with the tables in the direction's order. A rank-1
    graph with ONE entry off by 1e-9 relative is not rank-1 and stays unfound (no approximation)."""
    from gated_gcrnns_amd.graph import GraphOperator
    S = directed_rank1(N, GRAPH_SEED, kind)
    g = _cpu_graph(kind, N)
    _assert_directed(g, S)
    a, b = _assert_rank1(g, S)
    pat = S[0] != 0
    assert np.abs(np.outer(a, b) * pat - S[0]).max() <= 1e-12
    at, bt = g.rank1_factors(adjoint=True)
    assert np.array_equal(at, b) and np.array_equal(bt, a)
    assert np.abs(np.outer(at, bt) * pat.T - S[0].T).max() <= 1e-12
    r = special_nodes(N)
    assert all(b[n] == 0 and a[n] != 0 for n in r['no_in']) and all(a[n] == 0 and b[n] != 0 for n in r['no_out'])
    pf, pa = g.fused_plan_rank1(), g.fused_plan_rank1(adjoint=True)
    assert pf is not None and pa is not None and g.fused_plan_img16() is None
    assert np.array_equal(_dense_from_img16(pf, N), pat.T.astype(np.float64)) and np.array_equal(_dense_from_img16(pa, N), pat.astype(np.float64))
    for plan, src, dst in ((pf, a, b), (pa, b, a)):          # image holds src (.) v, the sums are scaled by dst
        assert np.array_equal(plan['rank1_a'].cpu().numpy()[:N], src.astype(np.float32))
        assert np.array_equal(plan['rank1_b'].cpu().numpy()[:N], dst.astype(np.float32))
    for adjoint, src, dst in ((False, a, b), (True, b, a)):   # x3 table: a | a b | 1 / b | b, 1 where b = 0
        tab = g.fused_plan_x3(adjoint=adjoint)['rank1_x3'].cpu().numpy()[:, :N].astype(np.float64)
        z = dst == 0
        assert z.any() and np.all(tab[2][z] == 1.0) and np.all(tab[3][z] == 1.0) and np.all(tab[1][z] == np.float32(1.0) * src[z].astype(np.float32))
        assert np.allclose(tab[0], src, rtol=1e-7, atol=0) and np.allclose(tab[3][~z], dst[~z], rtol=1e-7, atol=0)
        assert np.allclose(tab[1][~z], (src * dst)[~z], rtol=1e-7, atol=0) and np.allclose(tab[2][~z] * dst[~z], 1.0, rtol=2e-7, atol=0)
    # negatives: one entry of a well-connected row and column moved by 1e-9 relative; uniform weights on the same pattern
    rows, cols = np.nonzero(S[0])
    i = next(i for i in range(rows.size) if pat[rows[i]].sum() >= 4 and pat[:, cols[i]].sum() >= 4 and rows[i] != cols[i])
    S2 = np.array(S)
    S2[0, rows[i], cols[i]] *= 1.0 + 1e-9
    assert GraphOperator(S2).rank1_factors() is None
    assert _cpu_graph('uni', N).rank1_factors() is None
    # the same graph rounded to fp32 is found at fp32's precision (as before)
    assert GraphOperator(f32_round(S)).rank1_factors() is not None


# ------------------------------------------------------------------------------------------------------------ a. forward, bf16
@pytest.mark.gpu
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 4), (ONE_IN, 3, 3)])
@pytest.mark.parametrize('kernel,tg', [(k, tg) for k in ('wide', 'hop', 'seq16', 'step') for tg in (False, True) if not (k == 'hop' and tg)])
def test_directed_uniform_forward_matches_oracle(kernel, tg, shape, B, T, monkeypatch):
    """bf16 forward of the un-gated and the time-gated cell on a directed uniform-weight graph against the fp64 oracle, on each kernel
    that carries it: the wide sequence-resident kernel, the hand-allocated-hop kernel (un-gated only: it has no gated variant), the
    16-feature sequence-resident kernel, the chunk-parallel step kernel. Caller-packed input and last-state-only give the bits of the full forward."""
    from gated_gcrnns_amd import ops
    p = _problem('uni', shape, B, T, tg)
    mx, mn = _h_bounds(p)
    _assert_directed(p.graph, p.S)
    _assert_discriminates(p, mx)
    _setenv(monkeypatch, FORWARD_ENV[kernel])
    cell = _device_cell(p, torch.bfloat16)
    Xd, hd = _operands(p, torch.bfloat16)
    Gp = ops.fused_padded_inputs(p.F, p.G)
    assert cell.graph.fused_plan_img16() is not None
    if kernel in ('wide', 'hop'):
        assert ops.fused_wide_plan(cell.graph, B, T, p.N, p.F, Gp, p.K, not tg) is not None
        if tg:
            assert ops.fused_gate_pair_plan(cell.graph, B, T, p.N, p.F, Gp, p.K, True)[0] is not None
    else:
        assert ops.fused_wide_plan(cell.graph, B, T, p.N, p.F, Gp, p.K, not tg) is None
    with torch.no_grad():
        assert cell._use_fused(Xd, hd)
        H = cell(Xd, hd)
        Hl = cell(Xd, hd, last_only=True)
        monkeypatch.setenv('GCRNN_NO_INLINE_PACK', '1')
        H2 = cell(Xd, hd)
    assert H.dtype == torch.bfloat16 and tuple(H.shape) == (B, T, p.F, p.N)
    err = _check_h(kernel, H, p, mx, mn)
    if p.G != 1 and not tg:
        assert err[:, 0].max() <= 4.0e-3, err[:, 0].max()      # (the first step's bound of tests/test_wide.py)
    assert torch.equal(H, H2) and torch.equal(H[:, -1:], Hl)


# ------------------------------------------------------------------------------------------------------------ b. output head
def _head_weights(F, seed=0):
    """Head weights (fp32 values) with four dominant features and small, distinct, non-zero weights on all others: a dense random head
    averages the F state differences of a transposed graph away (7 .. 19 tolerances measured on the reference), while ||w||_1 -- and with
    it the bound -- grows with every feature; every feature still enters the sum with a weight of its own."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.005, 0.02, F) * rng.choice([-1.0, 1.0], F)
    w[rng.choice(F, 4, replace=False)] = np.array([1.0, -0.8, 0.6, -0.4])
    return f32_round(w)


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 4)])
def test_directed_uniform_wide_head_matches_oracle(shape, B, T, tg, monkeypatch):
    """ops.fused_cell_forward_wide_head (cell + Linear(F -> 1) as one launch) against w . H_oracle + b at ||w||_1 times the bound on H."""
    from gated_gcrnns_amd import ops
    p = _problem('uni', shape, B, T, tg)
    w = _head_weights(p.F)
    hb = float(np.float32(0.37))
    yref, yreft = np.einsum('f,btfn->btn', w, p.H) + hb, np.einsum('f,btfn->btn', w, p.Ht) + hb
    tol = float(np.abs(w).sum()) * _h_bounds(p)[0]
    _assert_directed(p.graph, p.S)
    _assert_discriminates(p, tol, 'the head', yref, yreft)
    _setenv(monkeypatch, FORWARD_ENV['wide'])
    cell = _device_cell(p, torch.bfloat16)
    Xd, hd = _operands(p, torch.bfloat16)
    dev = Xd.device
    assert ops.fused_wide_head_supported(cell.graph, B, T, p.N, p.F, ops.fused_padded_inputs(p.F, p.G), p.K, tg)
    head = (torch.tensor(w, dtype=torch.float32, device=dev).view(1, p.F), torch.tensor([hb], dtype=torch.float32, device=dev))
    with torch.no_grad():
        y = ops.fused_cell_forward_wide_head(Xd, hd, ops.fused_pad_taps(cell.weight_A), cell.weight_B, cell.bias, cell.graph, head,
                                             gates=cell._fused_gates() if tg else None)
    assert tuple(y.shape) == (B, T, 1, p.N) and y.dtype == torch.float32
    e = float(np.abs(y[:, :, 0].double().cpu().numpy() - yref).max())
    line = 'directed wide head N=%d tg=%s: |y - head(H_oracle)| max %.3e (bound %.3e)' % (p.N, tg, e, tol)
    print(line); _tol_report(line)
    assert e <= tol, (e, tol)


# ------------------------------------------------------------------------------------------------------------ c. node / edge gates
@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('sg', ['node', 'edge'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_spatially_gated_forward_matches_oracle(shape, B, T, sg, tg, monkeypatch):
    """Node-gated and edge-gated cells (with and without time gates) on the wide kernel's passes -- the all-items filter output, the
    node-gated recurrence, the gate-pair pre-pass, the edge-gated cell's per-step state filter -- against the fp64 oracle."""
    from gated_gcrnns_amd import _lib
    p = _problem('uni', shape, B, T, tg, sg)
    mx, mn = _h_bounds(p)
    _assert_directed(p.graph, p.S)
    _assert_discriminates(p, mx)
    _setenv(monkeypatch, {'GCRNN_SEQ32_MIN_B': '1'})
    cell = _device_cell(p, torch.bfloat16)
    Xd, hd = _operands(p, torch.bfloat16)
    p16 = cell.graph.fused_plan_img16()
    assert p16 is not None
    assert _lib.lib.gcrnn_fused_filter_output_wide_supported(B, 1 if sg == 'edge' else T, p.N, p.F, p.F, p.K, int(p16['entries']), float(p16['uniform_w']), 1, 0) == 1
    if sg == 'node':
        assert _lib.lib.gcrnn_fused_node_forward_wide_supported(B, T, p.N, p.F, p.K, int(p16['entries']), float(p16['uniform_w']), 1) == 1
    with torch.no_grad():
        assert cell._use_fused_node(Xd, hd) if sg == 'node' else cell._use_fused_edge(Xd, hd)
        H = cell(Xd, hd)
        Hl = cell(Xd, hd, last_only=True)
    _check_h('wide passes', H, p, mx, mn)
    assert torch.equal(H[:, -1:], Hl)


# ------------------------------------------------------------------------------------------------------------ d. training, bf16
# bf16 gradients: the class gates of tests/test_fused.py (5e-2 max, 1e-2 mean of the gradient's max through _grad_scale_and_bounds). A
# transposed graph moves d X, d h0 and weight_B's gradient by 0.34 .. 0.96 of their max -- under 20 x 5e-2 -- so THESE three, the ones that
# tell the plans apart, are held to 1.5e-2 (the ceiling the G9 fixture test keeps for a loss linear in H): 20 x 1.5e-2 = 0.30.
TIGHT_GRAD = 1.5e-2


def _train_and_check(tag, p, g, cell, Xd, hd, mx, mn, dx_dh0=(), ceilings=None, deferred=None):
    """One training step on loss = (H * dH).sum(); every parameter gradient (and dX / dh0 where asked) against the torch reference.
    ceilings {name: fraction of the max}: these gradients are asserted at their ceiling here, and what they miss of their bound is
    appended to `deferred` for the caller."""
    dHd = torch.tensor(p.dH, dtype=torch.float32, device=Xd.device)
    cell.zero_grad(set_to_none=True)
    Xd.grad = hd.grad = None
    H = cell(Xd, hd)
    (H.float() * dHd).sum().backward()
    got = {n: q.grad.double().cpu().numpy() for n, q in cell.named_parameters() if q.grad is not None}
    for n, q in cell.named_parameters():                  # parameters the reference leaves without gradient (the unused output gate)
        if n not in g:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, n
    if 'dX' in dx_dh0:
        got['dX'] = Xd.grad.double().cpu().numpy()
    if 'dh0' in dx_dh0:
        got['dh0'] = hd.grad.double().cpu().numpy()
    worst = (0.0, 0.0, None)
    checked, missed = 0, []
    for k, gr in g.items():
        if k in ('dX', 'dh0') and k not in dx_dh0:
            continue
        assert k in got, k
        e = np.abs(got[k] - gr)
        sc, tmax, tmean = float(np.abs(gr).max()), mx, mn
        if gr.size == 1 and k.endswith('.bias') and mx >= 5e-2:
            # bf16 only (tests/test_fused.py, node-gated training): a scalar bias is a signed sum that may cancel -- on its sibling weight's
            # scale. The x3 path holds every gradient, the scalar gate biases included, to 2e-5 of its OWN max (G11 / G12)
            sc = max(sc, float(np.abs(g.get(k[:-5] + '.weight', gr)).max()))
        elif k not in ('dX', 'dh0') and mx >= 5e-2:
            sc, tmax, tmean = _grad_scale_and_bounds(k, {n: v for n, v in g.items() if n not in ('dX', 'dh0')}, mx, mn)
        if k in ('weight_B', 'dX', 'dh0'):
            tmax = min(tmax, TIGHT_GRAD)
        assert sc > 0, k
        _tol_report('directed %s %s N=%d tg=%s sg=%s %s max %.3e mean %.3e (gate %.1e / %.1e)' % (tag, p.kind, p.N, p.tg, p.sg, k, e.max() / sc, e.mean() / sc, tmax, tmean))
        if e.max() / sc > worst[0]:
            worst = (e.max() / sc, e.mean() / sc, k)
        inside = e.max() <= tmax * sc and (e.size < 16 or e.mean() <= tmean * sc)
        if ceilings is not None and k in ceilings:
            if not inside:
                deferred.append('%s %s max %.3e mean %.3e (bounds %.1e / %.1e)' % (tag, k, e.max() / sc, e.mean() / sc, tmax, tmean))
            assert e.max() <= ceilings[k] * sc, (tag, k, e.max() / sc, ceilings[k])
        elif not inside:
            missed.append('%s max %.3e mean %.3e (bounds %.1e / %.1e)' % (k, e.max() / sc, e.mean() / sc, tmax, tmean))
        checked += 1
    print('directed %s %s N=%d tg=%s sg=%s: %d gradients, worst %s at %.3e of its max (mean %.3e; bounds %.1e / %.1e)' % (
        tag, p.kind, p.N, p.tg, p.sg, checked, worst[2], worst[0], worst[1], mx, mn))
    assert not missed, (tag, missed)                          # (every gradient is measured and reported before the first one fails the case)
    return H.detach(), checked


def _bf16_training(p, g, gt, monkeypatch, rank1=False, ceilings=None, deferred=None):
    from gated_gcrnns_amd import _lib, ops
    dev = torch.device('cuda:0')
    wants = ('dX', 'dh0') if p.sg is None else ()
    mx, mn = (8.0e-3, 1.2e-3) if rank1 else _h_bounds(p)      # (rank-1: tests/test_wide.py, training on rank-1-weighted graphs)
    _assert_grads_discriminate(g, gt, ('weight_B',) + wants, TIGHT_GRAD)
    _assert_discriminates(p, mx)
    cell = _device_cell(p, torch.float32)                   # fp32 master weights holding bf16-representable values
    Xd, hd = _operands(p, torch.bfloat16)
    Xd.requires_grad_(bool(wants)); hd.requires_grad_(bool(wants))
    pa = cell.graph.fused_plan_rank1(adjoint=True) if rank1 else cell.graph.fused_plan_img16(adjoint=True)
    assert pa is not None
    # (the flag the chain is asked with: on a uniform-weight graph the launch lays out the user-layout dH itself)
    inline = 1 if ops.fused_inline_pack_ok(cell.graph.fused_plan(adjoint=True), p.N, p.F, p.F, p.K) else 0
    assert inline == (0 if rank1 else 1)
    outs = []
    for chain in ('wide chain', '16-feature chain'):
        _setenv(monkeypatch, {'GCRNN_SEQ32_MIN_B': '1'} if chain == 'wide chain' else {'GCRNN_SEQ32_MIN_B': '1', 'GCRNN_NO_WIDE_CHAIN': '1', 'GCRNN_SEQ_MIN_B': '1'})
        assert cell._use_fused_training(Xd, hd)
        assert _lib.lib.gcrnn_fused_backward_data_wide_supported(p.B, p.T, p.N, p.F, p.K, int(pa['entries']), float(pa['uniform_w']), 3 if rank1 else 1, inline) == 1
        H, checked = _train_and_check(chain, p, g, cell, Xd, hd, 5e-2, 1e-2, wants, ceilings, deferred)
        assert checked >= {None: 3, 'node': 11, 'edge': 7}[p.sg] + (6 if p.tg else 0) + len(wants)
        outs.append(H)
    _check_h('training forward', outs[0], p, mx, mn)


@pytest.mark.gpu
@pytest.mark.parametrize('tg,sg', [(False, None), (True, None), (False, 'node')])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_training_matches_torch_reference(shape, B, T, tg, sg, monkeypatch):
    """bf16 activations over fp32 master weights on a directed uniform-weight graph: forward on the forward plan, BPTT chain, dX and
    the weight gradients on the adjoint plan -- every parameter gradient, and dX / dh0 where the fused path produces them (no spatial
    gates), against torch autograd in fp64; once with the chain as one launch of the wide kernel, once on the 16-feature chain."""
    p = _problem('uni', shape, B, T, tg, sg)
    g, gt = _grads('uni', shape, B, T, tg, sg)
    _assert_directed(p.graph, p.S)
    _bf16_training(p, g, gt, monkeypatch)


# Edge-gated training. On this graph some gradients of the edge-gated cell miss the bf16 class bounds (measured on an MI355X, of each
# gradient's max; the wide chain and the 16-feature chain give the same figures):
EDGE_KNOWN_MISSES = {
    400: ('weight_A', 'weight_B', 'bias', 'input_attention.weight'),
    1000: ('weight_B', 'forget_attention.weight'),
}
#   N = 400:  weight_A 6.2e-2 (bound 5e-2), weight_B 2.4e-2 (1.5e-2), bias mean 1.27e-2 (1e-2), input_attention.weight 1.06e-1 (8e-2)
#   N = 1000: weight_B 4.6e-2 (1.5e-2; inside the symmetric tests' 5e-2), forget_attention.weight 1.02e-1 (8e-2)
# The cause is the conditioning of the bf16 edge path behind the hub, not a plan or a direction: the fp64 reference with the filter
# outputs z rounded to bf16 before the attention -- no kernel at all -- already moves d X by 3.1e-2, weight_B by 2.1e-2 and
# forget_attention.weight by 8.7e-2 of their max (single ReLU / leaky-ReLU sign flips behind the hub's 125-way softmax); on the
# symmetrised pattern (A | A^T, same hub) the same cell measures weight_A 2.3e-2 .. 7.2e-2 and input_attention.weight up to 2.3e-1 over
# three parameter seeds; the worst entry of weight_A sits in tap 0, which no plan enters. Neither the issue's state-rounding emulation
# (weight_A: 1.4e-5) nor three times that z-rounding emulation (weight_A: 3 x 1.3e-2) covers every figure, so no bound is widened:
#   * test_directed_uniform_edge_gated_training asserts, with no mark, the predicates, the discrimination condition, every gradient that is
#     inside its bound AT its bound, and the listed ones at HALF of what a transposed graph moves them by in the reference (0.43 .. 1.16
#     of their max: a ceiling of 0.21 .. 0.58, which a launch on the other direction's plan cannot meet);
#   * test_directed_uniform_edge_gated_training_known_misses holds the listed ones to their bounds and is the expected failure: the
#     mark covers that one comparison (raises=AssertionError; anything else the case does fails it outright).
_EDGE_DEFERRED = {}


def _edge_gated_training(shape, B, T, monkeypatch):
    if shape not in _EDGE_DEFERRED:
        p = _problem('uni', shape, B, T, False, 'edge')
        g, gt = _grads('uni', shape, B, T, False, 'edge')
        _assert_directed(p.graph, p.S)
        names = [k for k in g if k not in ('dX', 'dh0')]
        _assert_grads_discriminate(g, gt, names, TIGHT_GRAD)      # (every edge-gated gradient, not weight_B alone)
        ceilings = {k: 0.5 * float(np.abs(g[k] - gt[k]).max()) / float(np.abs(g[k]).max()) for k in EDGE_KNOWN_MISSES[p.N]}
        deferred = []
        _bf16_training(p, g, gt, monkeypatch, ceilings=ceilings, deferred=deferred)
        _EDGE_DEFERRED[shape] = deferred
    return _EDGE_DEFERRED[shape]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_edge_gated_training(shape, B, T, monkeypatch):
    """The edge-gated cell's training step on the directed graph (both attention layers, forward and BPTT on the fused kernels): see
    EDGE_KNOWN_MISSES for what is asserted at which level."""
    _edge_gated_training(shape, B, T, monkeypatch)


@pytest.mark.gpu
@pytest.mark.xfail(strict=True, raises=AssertionError, reason='conditioning of the bf16 edge path behind the hub: weight_A 6.2e-2 of its max at N = 400 '
                   '(bound 5e-2), weight_B 4.6e-2 at N = 1000 (bound 1.5e-2); figures at EDGE_KNOWN_MISSES')
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_edge_gated_training_known_misses(shape, B, T, monkeypatch):
    """The listed gradients at the bounds the other cells meet (5e-2 / 1e-2 class gates, 1.5e-2 on weight_B)."""
    try:
        deferred = _edge_gated_training(shape, B, T, monkeypatch)
    except AssertionError as e:                                  # not the known miss: a real failure, outside the mark
        pytest.fail('edge-gated training failed before the deferred comparison: %s' % (e,))
    print('edge-gated training N=%d, outside their bounds: %s' % (shape[0], deferred))
    assert not deferred, deferred


# ------------------------------------------------------------------------------------------------------------ e. ops level
def _dense_filter(w, bias, Sd, x):
    """sum_k w_k (x Sd^k) + bias for x [items][C][N], w [F][1][K][C] -> [items][F][N] (fp64)."""
    y = np.zeros((x.shape[0], w.shape[0], x.shape[2]))
    z = x
    for k in range(w.shape[2]):
        y += np.einsum('fc,icn->ifn', w[:, 0, k, :], z)
        z = z @ Sd
    return y if bias is None else y + bias.reshape(1, -1, 1)


def _user_layout(a, N, zero_pad=False):
    """sequence-major [T][B][NPad][C] -> [B][T][C][N] fp64 on the host (zero_pad: the padding rows must be zero)."""
    assert not zero_pad or float(a[:, :, N:].float().abs().max()) == 0.0
    return a[:, :, :N].permute(1, 0, 3, 2).double().cpu().numpy()


# Ops-level bounds. The symmetric-graph tests allow 2.5e-2 of the max for the filter output and for the chain (tests/test_fused.py,
# tests/test_wide.py) and 2e-2 for dW; a transposed graph moves these references by 0.39 .. 0.69 of their max only (dW as a whole: 0.36,
# its tap 0 does not see S), so at those bounds the margin of 20 is not there. Tighter here, never wider:
FILTER_TOL = 2e-2          # of the output's max
DH0_TOL = (1.5e-2, 2e-3)   # d h0: max, mean of its max
WGRAD_TOL = 2e-2           # dW, tap by tap, of THAT tap's max (the taps k >= 1 are the ones that see S)
# dpre_t = (dH_t + c_t) (1 - h_t^2) is mostly its local term, which no graph enters: its bound is elementwise, the bf16 store of the element
# (half an ulp is 2^-9 |dpre|; twice that) plus d h0's 1.5e-2 on the CARRIED term's max, max |c_t (1 - h_t^2)|
DPRE_TOL = (2.0 ** -8, 1.5e-2)


@functools.lru_cache(maxsize=None)
def _filter_case(shape, B, T, adj):
    """Operands of one filter-output pass and its dense fp64 value on S (S^T for the adjoint pass) -- and on the other direction."""
    N, F, C, K = shape
    rng = np.random.default_rng(83 + N)
    w = bf16_round(0.2 * rng.standard_normal((F, 1, K, C)))
    bias = f32_round(0.1 * rng.standard_normal((F, 1)))
    x = bf16_round(rng.standard_normal((B, T, C, N)))
    S32 = f32_round(directed_uniform(N, GRAPH_SEED))[0]
    ref = _dense_filter(w, bias, S32.T if adj else S32, x.reshape(B * T, C, N)).reshape(B, T, F, N)
    reft = _dense_filter(w, bias, S32 if adj else S32.T, x.reshape(B * T, C, N)).reshape(B, T, F, N)
    return w, bias, x, ref, reft


@pytest.mark.gpu
@pytest.mark.parametrize('adj', [False, True])
@pytest.mark.parametrize('kernel', ['wide', 'seq16', 'step'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 2), (LARGE, 2, 2)])
def test_directed_uniform_filter_output_matches_dense(shape, B, T, kernel, adj, monkeypatch):
    """ops.fused_filter_output on the forward and on the adjoint plan against a dense fp64 evaluation of sum_k w_k (x S^k) + b (S^T for
    the adjoint), EVERY item: the direction is the only thing that tells the two plans apart."""
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator
    N, F, C, K = shape
    S = directed_uniform(N, GRAPH_SEED)
    w, bias, x, ref, reft = _filter_case(shape, B, T, adj)
    scale = float(np.abs(ref).max())
    tol = FILTER_TOL * scale
    assert float(np.abs(ref - reft).max()) >= MARGIN * tol, float(np.abs(ref - reft).max()) / scale
    dev = torch.device('cuda:0')
    graph = GraphOperator(S, device=dev)
    _assert_directed(graph, S)
    p16 = graph.fused_plan_img16(adjoint=adj)
    assert p16 is not None
    _setenv(monkeypatch, FORWARD_ENV[kernel])
    from gated_gcrnns_amd import _lib
    wide = _lib.lib.gcrnn_fused_filter_output_wide_supported(B, T, N, F, C, K, int(p16['entries']), float(p16['uniform_w']), 1, 0)
    assert wide == (1 if kernel == 'wide' else 0)               # the forced kernel is the one that runs
    xs = ops.to_sequence_major(torch.tensor(x, dtype=torch.bfloat16, device=dev), graph)
    out = ops.fused_filter_output(xs, torch.tensor(w, dtype=torch.float32, device=dev), torch.tensor(bias, dtype=torch.float32, device=dev),
                                  graph, K, N, adjoint=adj)
    per_item = np.abs(_user_layout(out, N, zero_pad=True) - ref).reshape(B * T, -1).max(axis=1) / scale
    line = 'directed filter output %s N=%d adjoint=%s: worst item %.3e of the max (bound %.1e)' % (kernel, N, adj, per_item.max(), FILTER_TOL)
    print(line); _tol_report(line)
    assert np.all(per_item <= FILTER_TOL), per_item


def _dense_dw(dpre, hprev, X, gf, Sd, K):
    """dW[f][k][:] = sum_{t,b,n} dpre_t[f][n] ([gf_t h_{t-1} | x_t] Sd^k)[:][n]: [F][K][F + G]."""
    B, T, F, N = dpre.shape
    z = np.concatenate([hprev * gf.T.reshape(B, T, 1, 1), X], axis=2).reshape(B * T, -1, N)
    dW = np.zeros((F, K, z.shape[1]))
    for k in range(K):
        dW[:, k, :] = np.einsum('ifn,icn->fc', dpre.reshape(B * T, F, N), z)
        z = z @ Sd
    return dW


@functools.lru_cache(maxsize=None)
def _chain_case(shape, B, T, gated):
    """The BPTT chain written out densely in fp64 on given states, upstream gradients and forget gates, for S and for S^T:
        dpre_t = (dH_t + c_t) (1 - h_t^2),  c_{t-1} = gf_t sum_k B_k^T dpre_t (S^T)^k  (c_T = 0; d h0 = c_{-1}),
        d gf_t = <B(S) h_{t-1} + b, dpre_t>,  and dW of the bf16-rounded dpre (what the weight-gradient kernel is handed)."""
    N, F, G, K = shape
    p = _problem('uni', shape, B, T)
    rng = np.random.default_rng(29 + N)
    Hs = bf16_round(np.tanh(rng.standard_normal((B, T, F, N))))
    gf = f32_round(rng.uniform(0.2, 0.9, (T, B))) if gated else np.ones((T, B))
    wB, bias = p.params['weight_B'], p.params['bias']
    wBt = np.ascontiguousarray(wB.transpose(3, 1, 2, 0))                       # [F_in][1][K][F_out]
    hprev = np.concatenate([p.h0[:, None], Hs[:, :-1]], axis=1)                # h_{t-1}
    out = []
    for Sd in (p.S32[0], np.ascontiguousarray(p.S32[0].T)):
        dpre = np.zeros((B, T, F, N))
        carry = np.zeros((B, F, N))
        for t in range(T - 1, -1, -1):
            dpre[:, t] = (p.dH[:, t] + carry) * (1.0 - Hs[:, t] ** 2)
            carry = gf[t].reshape(B, 1, 1) * _dense_filter(wBt, None, Sd.T, dpre[:, t])
        dgf = np.einsum('btfn,btfn->tb', _dense_filter(wB, bias, Sd, hprev.reshape(B * T, F, N)).reshape(B, T, F, N), dpre)
        dpre16 = bf16_round(dpre)
        cmax = float(np.abs(dpre - p.dH * (1.0 - Hs ** 2)).max())
        out.append(types.SimpleNamespace(dpre=dpre, dh0=carry, dgf=dgf, dpre16=dpre16, dpre_bound=DPRE_TOL[0] * np.abs(dpre) + DPRE_TOL[1] * cmax, dW=_dense_dw(dpre16, hprev, p.X, gf, Sd, K),
                                         db=((1.0 + gf.T).reshape(B, T, 1, 1) * dpre16).sum(axis=(0, 1, 3))))
    return p, Hs, gf, out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('chain', ['wide', 'seq16'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_backward_data_and_weight_match_dense(shape, B, T, chain, gated, monkeypatch):
    """ops.fused_backward_data (dpre of EVERY step, d h0, and the forget gate's gradient of the gated chain) and ops.fused_backward_weight
    on a directed uniform-weight graph -- both run on the ADJOINT plan -- against the dense fp64 chain of _chain_case."""
    from gated_gcrnns_amd import ops, _lib
    N, F, G, K = shape
    p, Hs, gf, r, rt = _chain_case(shape, B, T, gated)
    assert float((np.abs(r.dpre - rt.dpre) / r.dpre_bound).max()) >= MARGIN
    assert float(np.abs(r.dh0 - rt.dh0).max()) >= MARGIN * DH0_TOL[0] * float(np.abs(r.dh0).max())
    assert all(float(np.abs(r.dW[:, k] - rt.dW[:, k]).max()) >= MARGIN * WGRAD_TOL * float(np.abs(r.dW[:, k]).max()) for k in range(1, K))
    dev = torch.device('cuda:0')
    cell = _device_cell(p, torch.bfloat16)
    _assert_directed(cell.graph, p.S)
    p16 = cell.graph.fused_plan_img16(adjoint=True)
    _setenv(monkeypatch, {'GCRNN_SEQ32_MIN_B': '1'} if chain == 'wide' else {'GCRNN_SEQ32_MIN_B': '1', 'GCRNN_NO_WIDE_CHAIN': '1', 'GCRNN_SEQ_MIN_B': '1'})
    assert p16 is not None
    bf = lambda a: torch.tensor(a, dtype=torch.bfloat16, device=dev)
    dH, H, h0, Xd = bf(p.dH), bf(Hs), bf(p.h0), bf(p.X)
    hs = ops.to_sequence_major(H, cell.graph)
    h0s = ops.to_sequence_major(h0.view(B, 1, F, N), cell.graph)
    dHs, dHu = ops.fused_pack_upstream(dH, cell.graph, K)
    assert dHu is not None                                      # uniform-weight graph: the chain lays out the user-layout dH itself ...
    assert _lib.lib.gcrnn_fused_backward_data_wide_supported(B, T, N, F, K, int(p16['entries']), float(p16['uniform_w']), 1, 1) == 1      # ... and is asked so
    wBd = cell.weight_B.detach().float()
    gfd = torch.tensor(gf, dtype=torch.float32, device=dev) if gated else None
    if gated:
        dpre, dh0, dgf = ops.fused_backward_data(dHs, hs, wBd, cell.graph, want_dh0=True, gf=gfd, h0s=h0s, bias=cell.bias.detach().float(), dH_user=dHu)
    else:
        dpre, dh0 = ops.fused_backward_data(dHs, hs, wBd, cell.graph, want_dh0=True, dH_user=dHu)
    sc0 = float(np.abs(r.dh0).max())
    per_step = (np.abs(_user_layout(dpre, N) - r.dpre) / r.dpre_bound).max(axis=(0, 2, 3))
    e0 = np.abs(_user_layout(dh0.unsqueeze(0), N)[:, 0] - r.dh0) / sc0
    line = 'directed BPTT chain %s N=%d gated=%s: dpre at most %.3f of its elementwise bound (steps %s), dh0 max %.3e mean %.3e of its max (bounds %.1e / %.1e)' % (
        chain, N, gated, per_step.max(), np.round(per_step, 3).tolist(), e0.max(), e0.mean(), DH0_TOL[0], DH0_TOL[1])
    print(line); _tol_report(line)
    assert np.all(per_step <= 1.0), per_step
    assert e0.max() <= DH0_TOL[0] and e0.mean() <= DH0_TOL[1], (e0.max(), e0.mean())
    if gated:
        eg = float(np.abs(dgf.double().cpu().numpy() - r.dgf).max() / np.abs(r.dgf).max())
        print('directed BPTT chain %s N=%d: d gf max %.3e of its max (bound 2.5e-2)' % (chain, N, eg))
        assert eg <= 2.5e-2, eg
    # the weight gradient of the REFERENCE's dpre (bf16-rounded, laid out by the library's pack)
    gid = torch.ones((T, B), dtype=torch.float32, device=dev) if gated else None
    dW, db = ops.fused_backward_weight(ops.to_sequence_major(bf(r.dpre16), cell.graph), Xd, H, h0, cell.graph, F, G, K, want_bias=True, gi=gid, gf=gfd)
    ew = np.abs(dW.double().cpu().numpy() - r.dW).max(axis=(0, 2)) / np.abs(r.dW).max(axis=(0, 2))
    eb = float(np.abs(db.double().cpu().numpy() - r.db).max() / np.abs(r.db).max())
    line = 'directed weight gradient N=%d gated=%s: dW per tap %s of each tap max, bias %.3e (bound %.1e)' % (N, gated, ['%.2e' % v for v in ew], eb, WGRAD_TOL)
    print(line); _tol_report(line)
    assert np.all(ew <= WGRAD_TOL) and eb <= WGRAD_TOL, (ew, eb)


# ------------------------------------------------------------------------------------------------------------ f. fp32-accurate kernels
def _x3_predicate(cell, Xd, hd, p):
    if p.sg == 'node':
        return cell._use_fused_x3_node(Xd, hd)
    if p.sg == 'edge':
        return cell._use_fused_x3_edge(Xd, hd)
    return cell._use_fused_x3(Xd, hd, time_gated=p.tg)


@pytest.mark.gpu
@pytest.mark.parametrize('tg,sg', [(False, None), (True, None), (False, 'node'), (False, 'edge')])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_fp32_accurate_forward_matches_oracle_to_1e5(shape, B, T, tg, sg):
    """The x3 kernels (three bf16 planes per fp32 operand) on a directed uniform-weight graph: un-gated, time-, node- and edge-gated
    forward at the project's 1e-5 against the fp64 oracle on fp32-representable operands."""
    p = _problem('uni', shape, B, T, tg, sg, 'f32')
    _assert_directed(p.graph, p.S)
    _assert_discriminates(p, 1e-5)
    cell = _device_cell(p, torch.float32)
    Xd, hd = _operands(p, torch.float32)
    with torch.no_grad():
        assert _x3_predicate(cell, Xd, hd, p)
        H = cell(Xd, hd)
    assert H.dtype == torch.float32
    _check_h('x3 forward', H, p, 1e-5, 1e-5)


def _x3_training(p, g, gt):
    wants = () if p.tg else ('dh0',)                          # (the time-gated x3 training path hands h0 no gradient)
    _assert_grads_discriminate(g, gt, ('weight_B',) + wants, 2e-5)
    _assert_discriminates(p, 1e-5)
    cell = _device_cell(p, torch.float32)
    Xd, hd = _operands(p, torch.float32)
    hd.requires_grad_(bool(wants))
    assert cell._use_fused_x3_training(Xd, hd, time_gated=p.tg)
    H, checked = _train_and_check('x3 training', p, g, cell, Xd, hd, 2e-5, 2e-5, wants)
    assert H.dtype == torch.float32 and checked == (13 if p.tg else 3) + len(wants)
    _check_h('x3 training forward', H, p, 1e-5, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_uniform_fp32_accurate_training_matches_torch_reference(shape, B, T, tg):
    """x3 forward, x3 data chain on the adjoint plan and the exact-fp32 weight gradient, un-gated and time-gated: H to 1e-5, every
    gradient to 2e-5 of its max (the bound of the x3 training tests of tests/test_fused.py) against torch autograd in fp64."""
    p = _problem('uni', shape, B, T, tg, None, 'f32')
    g, gt = _grads('uni', shape, B, T, tg, None, 'f32')
    _assert_directed(p.graph, p.S)
    _x3_training(p, g, gt)


# ------------------------------------------------------------------------------------------------------------ g. rank-1 directed graphs
def _assert_zero_factor_nodes_are_exact(p, cell, Xd, hd, H, dtype):
    """Nodes whose destination factor is zero receive from nobody, nodes whose source factor is zero send to nobody -- EXACTLY, in the
    oracle and in the kernels alike: new inputs everywhere else leave the states at the no-in nodes bit for bit; new inputs at the
    no-out nodes change the states at those nodes and nowhere else."""
    r = special_nodes(p.N)
    rng = np.random.default_rng(3)
    rnd = bf16_round if dtype == torch.bfloat16 else f32_round
    keep = np.zeros(p.N, dtype=bool); keep[r['no_in']] = True
    X1 = np.where(keep, p.X, rnd(rng.standard_normal(p.X.shape)))
    h1 = np.where(keep, p.h0, rnd(0.3 * rng.standard_normal(p.h0.shape)))
    move = np.zeros(p.N, dtype=bool); move[r['no_out']] = True
    X2 = np.where(move, rnd(rng.standard_normal(p.X.shape)), p.X)
    h2 = np.where(move, rnd(0.3 * rng.standard_normal(p.h0.shape)), p.h0)
    O0 = orc.ggcrnn_cell(p.params, p.S32, p.X[:1], p.h0[:1])      # (one sequence each: same shapes, same order of every sum)
    O1 = orc.ggcrnn_cell(p.params, p.S32, X1[:1], h1[:1])
    O2 = orc.ggcrnn_cell(p.params, p.S32, X2[:1], h2[:1])
    assert np.array_equal(O1[..., keep], O0[..., keep]) and not np.array_equal(O1[..., ~keep], O0[..., ~keep])
    assert np.array_equal(O2[..., ~move], O0[..., ~move]) and not np.array_equal(O2[..., move], O0[..., move])
    dev = Xd.device
    with torch.no_grad():
        H1 = cell(torch.tensor(X1, dtype=dtype, device=dev), torch.tensor(h1, dtype=dtype, device=dev))
        H2 = cell(torch.tensor(X2, dtype=dtype, device=dev), torch.tensor(h2, dtype=dtype, device=dev))
    keep_d, move_d = torch.tensor(keep, device=dev), torch.tensor(move, device=dev)
    assert torch.equal(H1[..., keep_d], H[..., keep_d]) and not torch.equal(H1[..., ~keep_d], H[..., ~keep_d])
    assert torch.equal(H2[..., ~move_d], H[..., ~move_d]) and not torch.equal(H2[..., move_d], H[..., move_d])


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['out', 'in', 'sym'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_rank1_wide_forward_matches_oracle(shape, B, T, kind, monkeypatch):
    """The wide kernel's rank-1 variant (image a (.) v on the PATTERN's forward plan, sums scaled by b) on the three normalisations of a
    directed pattern, given in fp64, against the fp64 oracle on the dense weighted S; zero-factor nodes exact."""
    from gated_gcrnns_amd import ops
    p = _problem(kind, shape, B, T)
    _assert_directed(p.graph, p.S)
    _assert_rank1(p.graph, p.S)
    _assert_discriminates(p, 5.0e-3)
    _setenv(monkeypatch, {'GCRNN_SEQ32_MIN_B': '1'})
    cell = _device_cell(p, torch.bfloat16)
    Xd, hd = _operands(p, torch.bfloat16)
    assert cell.graph.fused_plan_img16() is None and cell.graph.fused_plan_rank1() is not None
    # (at N = 1000 the hub makes the forward plan of the pattern 828 entries deep: next to the two factor tables the LDS has no room
    # for the inline layout of X, and the launch takes the caller-packed input)
    assert ops.fused_wide_plan(cell.graph, B, T, p.N, p.F, p.G, p.K, False, rank1=True) is not None
    with torch.no_grad():
        H = cell(Xd, hd)
        Hl = cell(Xd, hd, last_only=True)
    err = _check_h('rank-1 wide', H, p, 5.0e-3, 1.0e-3)
    assert err[:, 0].max() <= 4.0e-3 and torch.equal(H[:, -1:], Hl)
    _assert_zero_factor_nodes_are_exact(p, cell, Xd, hd, H, torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['out', 'in', 'sym'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_rank1_fp32_accurate_forward_matches_oracle_to_1e5(shape, B, T, kind):
    """The x3 kernels on the factor table a | a b | 1 / b | b (1 where b = 0 -- nodes nobody sends to, which only a directed graph has next
    to a non-zero a) at 1e-5 against the fp64 oracle; zero-factor nodes exact."""
    p = _problem(kind, shape, B, T, False, None, 'f32')
    _assert_directed(p.graph, p.S)
    _assert_rank1(p.graph, p.S)
    _assert_discriminates(p, 1e-5)
    cell = _device_cell(p, torch.float32)
    Xd, hd = _operands(p, torch.float32)
    assert cell.graph.fused_plan_x3().get('rank1_x3') is not None
    with torch.no_grad():
        assert cell._use_fused_x3(Xd, hd)
        H = cell(Xd, hd)
    _check_h('rank-1 x3', H, p, 1e-5, 1e-5)
    _assert_zero_factor_nodes_are_exact(p, cell, Xd, hd, H, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('kind', ['out', 'in', 'sym'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_rank1_wide_training_matches_torch_reference(shape, B, T, kind, tg, monkeypatch):
    """bf16 training on the rank-1 variants: forward with (a, b) on the pattern's forward plan, the BPTT chain and the weight gradient
    with the SWAPPED factors on its adjoint plan -- swapped factors or a swapped plan show in the pattern here, not only in the values."""
    p = _problem(kind, shape, B, T, tg)
    g, gt = _grads(kind, shape, B, T, tg)
    _assert_directed(p.graph, p.S)
    _assert_rank1(p.graph, p.S)
    _bf16_training(p, g, gt, monkeypatch, rank1=True)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['out', 'in', 'sym'])
@pytest.mark.parametrize('shape,B,T', [(SMALL, 3, 3), (LARGE, 2, 3)])
def test_directed_rank1_fp32_accurate_training_matches_torch_reference(shape, B, T, kind):
    """x3 training on a directed rank-1 graph: H to 1e-5, every gradient (d h0 included) to 2e-5 of its max."""
    p = _problem(kind, shape, B, T, False, None, 'f32')
    g, gt = _grads(kind, shape, B, T, False, None, 'f32')
    _assert_directed(p.graph, p.S)
    _assert_rank1(p.graph, p.S)
    assert p.graph.fused_plan_x3(adjoint=True).get('rank1_x3') is not None
    _x3_training(p, g, gt)
