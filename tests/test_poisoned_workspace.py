"""Every kernel path on poisoned work buffers (tests/poison.py).

Every device buffer of the library comes from torch.empty, and most are larger than what the kernels write: padded node rows
([..][NPad = 1024][C] for N <= 1024), inputs of which only the leading steps are laid out, raw scratch, per-slot partial sums, rotating
planes. The kernels rest on what the unwritten part holds ("rows >= N are zero"), a fresh process mostly gets zeroed pages, and the
bit-identity tests run one problem twice in a row, so the second run gets the first run's block with the right data in it. Here each case
builds its whole problem from seeds and runs it three times, with torch.empty returning zeros, NaN and 1.5 * 2^100: every output is finite
and the three runs agree bit for bit (poison.assert_independent_of_workspace). So that three equal wrong results cannot pass, the run on
zeros is also held to the same cell in fp64 on the composed path (copy.deepcopy(cell).double() with an activation the kernel predicates do
not recognise), which is pinned once per gating to oracle/torch_reference.py, at the bound the existing test of that kernel carries.

A case that fails is a finding about the library: DESIGN.md, "What kernels may assume about work buffers"."""
import copy
import functools
import os
import types

import numpy as np
import pytest
import torch

from poison import BIG, FILLS, assert_independent_of_workspace, poisoned_allocations

DEV = torch.device('cuda:0')


# ================================================================================================================== CPU: the harness
def _allocators():
    return torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty


def test_allocators_are_the_original_objects_again_after_the_block():
    before = _allocators()
    shadowed = 'new_empty' in torch.Tensor.__dict__
    with poisoned_allocations('nan') as counter:
        inside = _allocators()
        assert all(a is not b for a, b in zip(inside, before))
        assert bool(torch.empty(3).isnan().all()) and counter.tensors == 1 and counter.bytes == 12
    assert all(a is b for a, b in zip(_allocators(), before))
    assert ('new_empty' in torch.Tensor.__dict__) == shadowed
    with pytest.raises(KeyError):
        with poisoned_allocations('big'):
            assert torch.empty is not before[0]
            raise KeyError('the body raises')
    assert all(a is b for a, b in zip(_allocators(), before))
    assert ('new_empty' in torch.Tensor.__dict__) == shadowed
    with pytest.raises(AssertionError):
        with poisoned_allocations('ones'):
            pass
    assert all(a is b for a, b in zip(_allocators(), before))


@pytest.mark.parametrize('fill', FILLS)
def test_dtype_policy(fill):
    """Floating dtypes and uint8 (the raw work buffers, which hold bf16) are filled; every other integer dtype and bool pass through, so
    no pattern can become an index. The dtypes are those of the package's torch.empty sites (bf16, fp32, fp64, uint8, int32, int64) and
    their neighbours."""
    floats = (torch.bfloat16, torch.float16, torch.float32, torch.float64)
    with poisoned_allocations(fill) as counter:
        n = 0
        for dt in floats:
            t = torch.empty(5, 3, dtype=dt)
            n += 1
            assert counter.tensors == n and t.dtype == dt
            if fill == 'zero':
                assert bool((t == 0).all())
            elif fill == 'nan':
                assert bool(t.isnan().all())
            else:
                assert bool(torch.isfinite(t).all()) and bool((t.double() >= 2.0 ** 15).all())
                if dt != torch.float16:
                    assert bool((t.double() == BIG).all())
        raw = torch.empty(64, dtype=torch.uint8)
        n += 1
        assert counter.tensors == n and counter.bytes == 15 * (2 + 2 + 4 + 8) + 64
        assert bool((raw == {'zero': 0x00, 'nan': 0xFF, 'big': 0x70}[fill]).all())
        for view in (torch.bfloat16, torch.float32, torch.float64):
            v = raw.view(view).double()
            if fill == 'zero':
                assert bool((v == 0).all())
            elif fill == 'nan':
                assert bool(v.isnan().all())
            elif view != torch.float64:
                assert bool(torch.isfinite(v).all()) and bool((v > 1e29).all()) and bool((v < 1e30).all())
        for dt in (torch.int8, torch.int16, torch.int32, torch.int64, torch.bool, torch.complex64):
            t = torch.empty(7, dtype=dt)
            assert t.dtype == dt and counter.tensors == n, dt
        assert torch.empty(0).numel() == 0 and counter.tensors == n


def test_positional_and_keyword_forms_behave_as_torchs():
    x = torch.arange(6.0).reshape(2, 3)
    with poisoned_allocations('nan') as counter:
        for t in (torch.empty(2, 3), torch.empty((2, 3)), torch.empty([2, 3]), torch.empty(size=(2, 3)), torch.empty(torch.Size((2, 3)))):
            assert tuple(t.shape) == (2, 3) and t.dtype == torch.float32 and bool(t.isnan().all())
        t = torch.empty((4,), dtype=torch.float64, device='cpu')
        assert t.dtype == torch.float64 and t.device.type == 'cpu' and bool(t.isnan().all())
        t = torch.empty(2, 2, dtype=torch.bfloat16, device=torch.device('cpu'), requires_grad=True)
        assert t.requires_grad and t.is_leaf and t.grad_fn is None and bool(t.detach().isnan().all())
        buf = torch.full((3,), 7.0)
        n = counter.tensors
        r = torch.empty(3, out=buf)                              # out=: the caller's storage, untouched
        assert r is buf and bool((buf == 7.0).all()) and counter.tensors == n
        t = torch.empty_like(x)
        assert t.shape == x.shape and t.dtype == x.dtype and bool(t.isnan().all()) and bool((x == torch.arange(6.0).reshape(2, 3)).all())
        t = torch.empty_like(x, dtype=torch.float64)
        assert t.dtype == torch.float64 and bool(t.isnan().all())
        n = counter.tensors
        assert torch.empty_like(x, dtype=torch.int32).dtype == torch.int32 and counter.tensors == n
        t = torch.empty_like(x.t())                              # preserve_format: the strides of the transposed view
        assert t.stride() == x.t().stride() and bool(t.isnan().all())
        t = torch.empty_strided((2, 3), (1, 2))
        assert t.stride() == (1, 2) and bool(t.isnan().all())
        t = torch.empty_strided(size=(2, 3), stride=(3, 1), dtype=torch.float64)
        assert t.dtype == torch.float64 and bool(t.isnan().all())
        for t in (x.new_empty((2, 2)), x.new_empty(2, 2), x.new_empty([2, 2])):
            assert tuple(t.shape) == (2, 2) and t.dtype == x.dtype and bool(t.isnan().all())
        t = x.new_empty((5,), dtype=torch.float64)
        assert t.dtype == torch.float64 and bool(t.isnan().all())
        n = counter.tensors
        assert x.new_empty((5,), dtype=torch.int64).dtype == torch.int64 and counter.tensors == n
        # what the package's modules do under the patch keeps working: parameters are allocated with torch.empty and then initialised
        torch.manual_seed(0)
        lin = torch.nn.Linear(4, 2)
        assert bool(torch.isfinite(lin.weight).all()) and bool(torch.isfinite(lin.bias).all())
        assert torch.equal(torch.stack((x, x)), torch.stack((x, x), out=torch.empty(2, 2, 3)))
    torch.manual_seed(0)
    ref = torch.nn.Linear(4, 2)
    assert torch.equal(lin.weight, ref.weight) and torch.equal(lin.bias, ref.bias)


def test_harness_rejects_a_result_that_reads_an_unwritten_buffer():
    with pytest.raises(AssertionError) as e:
        assert_independent_of_workspace(lambda: {'total': torch.empty(8).sum()})
    assert "'total'" in str(e.value)
    with pytest.raises(AssertionError) as e:                    # finite fills only: the message names output, fills and index
        assert_independent_of_workspace(lambda: {'v': torch.arange(6.0).reshape(2, 3) + torch.empty(2, 3) * torch.tensor([[0, 0, 0], [0, 1.0, 1.0]])},
                                        fills=('zero', 'big'))
    msg = str(e.value)
    assert "'v'" in msg and "'zero'" in msg and "'big'" in msg and '(1, 1)' in msg, msg
    with pytest.raises(AssertionError) as e:                    # a case that allocates nothing is a broken case
        assert_independent_of_workspace(lambda: {'x': torch.zeros(3)})
    assert 'allocated nothing' in str(e.value)


def test_harness_accepts_a_result_that_does_not():
    def run():
        buf = torch.empty(8)
        buf.copy_(torch.arange(8.0))
        return {'total': (torch.zeros(8) + buf).sum()}
    runs = assert_independent_of_workspace(run)
    assert sorted(runs) == sorted(FILLS) and all(float(r['total']) == 28.0 for r in runs.values())


# ================================================================================================================== GPU: negative control
@pytest.mark.gpu
def test_harness_rejects_an_accumulating_spmm_into_an_unwritten_output():
    """ops.spmm_raw(csr, X, out=torch.empty_like(X), accumulate=True): a caller error the API permits; the result is the fill plus S X.
    The N = 37 graph of test_streaming_spmm_edge_cases. Float data only: nothing can fault."""
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import operator_from_csr
    N = 37
    rng = np.random.default_rng(2)
    deg = rng.integers(0, 6, size=N)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = np.concatenate([np.sort(rng.choice(N, size=d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.uniform(-1, 1, col.size)

    def run(out_of):
        g = operator_from_csr(rowptr, col, val, N, device=DEV)
        X = torch.tensor(np.random.default_rng(3).standard_normal((2, N, 8)), dtype=torch.float32, device=DEV)
        return {'Y': ops.spmm_raw(g.fwd[0], X, out=out_of(X), accumulate=True)}
    with pytest.raises(AssertionError) as e:
        assert_independent_of_workspace(lambda: run(torch.empty_like))
    assert "'Y'" in str(e.value)
    with pytest.raises(AssertionError) as e:
        assert_independent_of_workspace(lambda: run(torch.empty_like), fills=('zero', 'big'))
    assert "'Y'" in str(e.value) and 'differ first at index (0, 0, 0)' in str(e.value)

    def ok():                                                   # the same call on an output the caller did write
        out = run(torch.zeros_like)
        out['scratch'] = torch.empty(4, device=DEV).zero_()     # (the counter must see something)
        return out
    assert_independent_of_workspace(ok)


# ================================================================================================================== GPU: the cell's paths
GATINGS = {'none': (False, None), 'time': (True, None), 'node': (False, 'node'), 'time+node': (True, 'node'), 'edge': (False, 'edge')}
#          name       N     F   G   K  B    T
SHAPES = {'U400': (400, 32, 32, 3, 4, 3),           # 624 padding rows, one 32-feature chunk
          'U1000': (1000, 64, 64, 5, 3, 4),         # 24 padding rows, partial last staged columns
          'U1008': (1008, 64, 64, 5, 260, 3),       # exactly the 16 padding rows the uniform plan needs; more sequences than CUs
          'U204': (204, 64, 64, 3, 3, 3),           # N % 8 != 0: _unpack_states instead of the direct user store
          'G1': (1000, 64, 1, 3, 3, 3),             # channels padded by pack_seq_major_padded
          'F20': (1000, 20, 1, 5, 4, 3),            # the padded-state cell (_state_padded)
          'X400': (400, 32, 32, 4, 3, 3),           # the fp32-accurate kernels' shapes
          'X1000': (1000, 64, 64, 5, 3, 3),
          'S1500': (1500, 32, 32, 3, 3, 3)}         # beyond the LDS-resident kernels: streaming
GRAPH_SEED = 71
# Training at U1000 runs B = 4, T = 3, the sizes of the N = 1000 training case of tests/test_wide.py (gate-pair training). The time gates'
# sub-cell biases GFL_in.bias / GFL_forget.bias are the one gradient class that sits AT the class gate (5e-2 max, 1e-2 mean of its max):
# a sum over nodes of terms weighted by the read-out's random-sign weights, which cancels to a small multiple of one term, while their
# sibling taps measure 2e-3 .. 6e-3. Measured (max / mean of the gradient's max), both chains alike since the error is made in the gates'
# own BPTT -- time+node-gated cell: B,T = 3,4 5.3e-2 / 1.6e-2; 3,3 5.8e-2 / 1.6e-2; 5,3 3.9e-2 / 1.2e-2; 4,3 4.5e-3 / 1.4e-3; time-gated
# cell: 3,4 3.8e-2 / 1.01e-2; 4,3 2.4e-2 / 7.7e-3. The figure follows how far that sum happens to cancel, not the kernels; the bound is
# not moved, and every other gradient of these cases sits a factor of 5 or more inside it.
TRAIN_BT = {'U400': (4, 3), 'U1000': (4, 3)}
_PINNED = set()


def _tanh(v):
    """tanh as a function object the cell's kernel predicates do not recognise (they ask `sigma in (torch.tanh, F.tanh)`): a cell with
    this activation runs the composed path, whatever its shape and dtype."""
    return torch.tanh(v)


@functools.lru_cache(maxsize=None)
def _gso(kind, N):
    """The graphs, built once (numpy arrays: no plan, pack or scratch lives here; every run makes its own GraphOperator from them)."""
    from test_wide import _normalized_adjacency, _uniform_cell
    if kind == 'uniform':
        S = _uniform_cell(N, 1, 1, 1, GRAPH_SEED)[2]
    elif kind == 'rank1':
        S = _normalized_adjacency(N, GRAPH_SEED, 'sym')[0]
    elif kind == 'weighted':                                    # arbitrary weights on the uniform graph's support: the weight image is used
        rng = np.random.default_rng(GRAPH_SEED + 1)
        R = np.triu(rng.uniform(0.5, 1.0, (N, N)), 1)
        W = (_gso('uniform', N)[0] != 0) * (R + R.T)
        S = (W / np.max(np.abs(np.linalg.eigvalsh(W)))).reshape(1, N, N)
    elif kind == 'adj59':
        from test_small_edge import gso_adj59
        S = np.array(gso_adj59(), dtype=np.float64)
    elif kind == 'dir17':
        from test_small_edge import gso_dir17
        S = gso_dir17()
    elif kind == 'g3':                                          # the graph of the g3_cell_* fixtures
        from conftest import load_golden
        S = load_golden('g3_cell_none')['S']
    else:
        raise KeyError(kind)
    S = np.ascontiguousarray(S, dtype=np.float64)
    S.setflags(write=False)
    return S


class Case(object):
    """One path. kind: what is called ('cell', 'head', 'train_head', 'native', 'classify', 'regress'); prec: 'bf16' (bf16 parameters),
    'master' (fp32 master weights holding bf16 values, bf16 activations), 'f32', 'f64'; mode: 'infer' / 'train'."""

    def __init__(self, id, path, shape, gating, graph='uniform', prec='bf16', mode='infer', env=None, kernel=None, route=None, bounds=None,
                 last_only=False, hz=False, dx=False, dh0=False, self_start=False, dims=None, sigma=None, family=None, pick=None, **kw):
        self.id, self.path, self.gating, self.graph, self.prec, self.mode = id, path, gating, graph, prec, mode
        self.tg, self.sg = GATINGS[gating]
        if dims is None:
            N, F, G, K, B, T = SHAPES[shape]
            if path == 'train':
                B, T = TRAIN_BT[shape]
            dims = dict(N=N, F=F, G=G, Kin=K, Kst=K, B=B, T=T)
        self.__dict__.update(dims)
        self.K = max(self.Kin, self.Kst)
        self.shape = shape
        self.env = dict(env or {})
        self.kernel, self.route, self.bounds = kernel, route, bounds
        self.last_only, self.hz, self.dx, self.dh0, self.self_start = last_only, hz, dx, dh0, self_start
        self.sigma, self.family, self.pick = sigma, family, pick
        self.kind = kw.pop('kind', 'cell')
        self.seed = kw.pop('seed', 89)
        self.O = kw.pop('O', 1)
        assert not kw, kw

    @property
    def xdtype(self):
        return {'bf16': torch.bfloat16, 'master': torch.bfloat16, 'f32': torch.float32, 'f64': torch.float64}[self.prec]


def _build(c, dev=None):
    """Cell, inputs and upstream gradient from seeds: the same values every time it is called."""
    import gated_gcrnns_amd.Utils.graphML as gml
    dev = DEV if dev is None else dev
    S = _gso(c.graph, c.N)
    torch.manual_seed(c.seed)
    tg = c.tg and c.kind != 'native'                            # (the stack: forward_native is the un-gated cell's; the gating is the second cell's)
    cell = gml.GGCRNNCell(c.G, c.F, c.Kin, c.Kst, torch.tanh if c.sigma is None else c.sigma, tg, c.sg, 1, True)
    cell.addGSO(torch.tensor(np.array(S)))
    if c.path == 'small':                                       # a contracting recurrence and gates away from 0.5 (tests/test_small_input_grad.py)
        from test_small_input_grad import _init
        _init(cell, c.G, c.F, c.Kin, c.Kst)
    elif tg:
        with torch.no_grad():                                   # make the scalar gates vary (tests/test_wide.py, tests/test_directed_uniform.py)
            scale = 8.0 if c.prec in ('bf16', 'master') else 6.0
            cell.MLP_in[0].weight.mul_(scale)
            cell.MLP_forget[0].weight.mul_(scale)
    if c.prec in ('bf16', 'master'):
        cell = cell.to(torch.bfloat16)
        if c.prec == 'master':
            cell = cell.float()
    else:
        cell = cell.to(c.xdtype)
    cell = cell.to(dev)
    g = torch.Generator().manual_seed(c.seed + 1)
    dt = c.xdtype
    if c.B > 64:                                                # (a full batch: drawn on the device, from the device's seeded generator)
        gd = torch.Generator(device=dev).manual_seed(c.seed + 1)
        X = torch.randn(c.B, c.T, c.G, c.N, generator=gd, dtype=torch.float32, device=dev).to(dt)
        h0 = (0.3 * torch.randn(c.B, c.F, c.N, generator=gd, dtype=torch.float32, device=dev)).to(dt)
    else:
        X = torch.randn(c.B, c.T, c.G, c.N, generator=g, dtype=torch.float64).to(dt).to(dev)
        h0 = (0.3 * torch.randn(c.B, c.F, c.N, generator=g, dtype=torch.float64)).to(dt).to(dev)
    if c.hz:
        h0 = torch.zeros_like(h0)
    up = torch.float32 if dt == torch.bfloat16 else dt          # the upstream gradient multiplies H.float() on the bf16 paths
    n_out = {'classify': (c.B, c.O), 'regress': (c.B, c.T, c.O, c.N), 'train_head': (c.B, c.T, 1, c.N), 'head': (c.B, c.T, 1, c.N)}.get(
        c.kind, (c.B, 1 if c.last_only else c.T, c.F, c.N))
    dOut = torch.randn(*n_out, generator=g, dtype=torch.float64).to(up).to(dev) if c.mode == 'train' else None
    head = None
    if c.kind in ('head', 'train_head'):
        from test_directed_uniform import _head_weights
        head = [torch.tensor(_head_weights(c.F), dtype=torch.float32, device=dev).view(1, c.F), torch.tensor([0.37], dtype=torch.float32, device=dev)]
    elif c.kind == 'classify':
        head = [(torch.randn(c.O, c.F * c.N, generator=g, dtype=torch.float64) / np.sqrt(c.F * c.N)).to(dt).to(dev),
                torch.randn(c.O, generator=g, dtype=torch.float64).to(dt).to(dev)]
    elif c.kind == 'regress':
        head = [(torch.randn(c.O, c.F, generator=g, dtype=torch.float64) / np.sqrt(c.F)).to(dt).to(dev),
                torch.randn(c.O, generator=g, dtype=torch.float64).to(dt).to(dev)]
    cell2 = None
    if c.kind == 'native':                                      # the second cell of the stack: F -> F, its own seed
        torch.manual_seed(c.seed + 7)
        cell2 = gml.GGCRNNCell(c.F, c.F, c.Kin, c.Kst, torch.tanh, c.tg, None, 1, True)
        cell2.addGSO(torch.tensor(np.array(S)))
        if c.tg:
            with torch.no_grad():
                cell2.MLP_in[0].weight.mul_(8.0)
                cell2.MLP_forget[0].weight.mul_(8.0)
        cell2 = cell2.to(torch.bfloat16).to(dev)
    return types.SimpleNamespace(cell=cell, cell2=cell2, X=X, h0=h0, dOut=dOut, head=head, S=S)


def _grads_of(p, cell, head, X, h0, c):
    out = {}
    for n, q in cell.named_parameters():
        if q.grad is not None:
            out['grad:' + n] = q.grad
    if head is not None and c.mode == 'train':
        out['grad:head.weight'], out['grad:head.bias'] = head[0].grad, head[1].grad
    if c.dx:
        out['grad:X'] = X.grad
    if c.dh0:
        out['grad:h0'] = h0.grad
    return out


def _apply_head(c, H, head):
    """The read-outs in plain torch, on the states of the reference cell."""
    w, b = head
    if c.kind in ('head', 'train_head'):
        return torch.einsum('of,btfn->bton', w, H) + b.view(1, 1, 1, 1)
    if c.kind == 'classify':
        return H[:, -1].reshape(H.shape[0], -1) @ w.t() + b
    return torch.einsum('of,btfn->bton', w, H) + b.view(1, 1, -1, 1)


def _native_stack(c, p):
    """Two stacked cells on the kernels' own layout: cell 1's sequence-major states, padding rows included, are cell 2's input."""
    from gated_gcrnns_amd import ops
    graph = p.cell.graph
    xs = ops.to_sequence_major(p.X, graph)
    h0s = ops.to_sequence_major(p.h0.view(c.B, 1, c.F, c.N), graph)[0]
    hs1 = p.cell.forward_native(xs, h0s)                        # [T][B][NPad][F]
    assert tuple(hs1.shape) == (c.T, c.B, graph.fused_plan()['npad'], c.F)
    c2 = p.cell2
    if not c.tg:
        hs2 = c2.forward_native(hs1.contiguous(), h0s)
        H = hs2.permute(1, 0, 3, 2)[..., :c.N].contiguous()
    else:                                                       # time-gated second cell: the packed operands are cell 1's image and a fresh state image
        hs_all = torch.empty((c.T + 1,) + tuple(hs1.shape[1:]), dtype=torch.bfloat16, device=hs1.device)
        hs_all[0].copy_(h0s)
        Xv = hs1.permute(1, 0, 3, 2)[..., :c.N]                 # (shapes only: with packed= the launches read xs)
        H = ops.fused_cell_forward(Xv, p.h0, c2.weight_A, c2.weight_B, c2.bias, c2.graph, gates=c2._fused_gates(), packed=(hs1.contiguous(), hs_all))
    return {'H1': hs1.permute(1, 0, 3, 2)[..., :c.N].contiguous(), 'H': H}


def _run_kernels(c, p=None):
    """What assert_independent_of_workspace runs under each fill. p: a problem built before (tests/test_sequence_isolation.py runs one build
    several times, on inputs of its own)."""
    p = _build(c) if p is None else p
    cell, X, h0 = p.cell, p.X, p.h0
    if c.mode == 'infer':
        with torch.no_grad():
            if c.route is not None:
                c.route(c, cell, X, h0)
            if c.kind == 'native':
                return _native_stack(c, p)
            if c.kind == 'head':
                from gated_gcrnns_amd import ops
                y = ops.fused_cell_forward_wide_head(X, h0, ops.fused_pad_taps(cell.weight_A), cell.weight_B, cell.bias, cell.graph, tuple(p.head),
                                                     gates=cell._fused_gates() if c.tg else None, self_start=c.self_start)
                return {'y': y}
            if c.kind in ('classify', 'regress'):
                y = getattr(cell, c.kind)(X, h0, *p.head)
                assert y is not None, 'the small-graph head path did not take the case'
                return {'y': y}
            return {'H': cell(X, h0, last_only=True) if c.last_only else cell(X, h0)}
    X.requires_grad_(c.dx)
    h0.requires_grad_(c.dh0)
    if p.head is not None:
        for t in p.head:
            t.requires_grad_(True)
    if c.route is not None:
        c.route(c, cell, X, h0)
    if c.kind == 'cell':
        out = cell(X, h0)
        name = 'H'
    elif c.kind == 'train_head':
        out = cell.train_with_head(X, h0, *p.head)
        name = 'y'
    else:
        out = getattr(cell, c.kind)(X, h0, *p.head)
        name = 'y'
    assert out is not None, 'the %s path did not take the case' % c.kind
    ((out.float() if out.dtype == torch.bfloat16 else out) * p.dOut).sum().backward()
    res = {name: out.detach()}
    res.update(_grads_of(p, cell, p.head, X, h0, c))
    return res


@functools.lru_cache(maxsize=None)
def _shape_sweep():
    """tools/shape_sweep.py (pin_cell_to_torch_reference), loaded from its file as tests/test_wide.py does."""
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('shape_sweep', os.path.join(ROOT, 'tools', 'shape_sweep.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _torch_reference(c, p):
    """The composed path has no other implementation of itself to be compared with: its truth is oracle/torch_reference.py directly
    (dense S, torch's own ops, autograd)."""
    from oracle import torch_reference as tr
    P = {k: v.detach().double().clone().requires_grad_(True) for k, v in p.cell.state_dict().items()}
    X, h0 = p.X.double().requires_grad_(c.dx), p.h0.double().requires_grad_(c.dh0)
    H = tr.ggcrnn_cell(P, torch.tensor(np.array(p.S), dtype=torch.float64, device=X.device), X, h0, c.tg, c.sg)
    (H * p.dOut.double()).sum().backward()
    res = {'H': H.detach()}
    res.update({'grad:' + k: v.grad for k, v in P.items() if v.grad is not None})
    res['grad:X'], res['grad:h0'] = X.grad, h0.grad
    return {k: v.detach().cpu() for k, v in res.items()}, slice(None)


def _run_reference(c):
    """The same cell as copy.deepcopy(cell).double() on the composed path, heads in plain torch; autograd gives every gradient. The fp64
    cell itself is pinned to oracle/torch_reference.py once per (path, gating, graph)."""
    p = _build(c)
    if c.path == 'composed':
        return _torch_reference(c, p)
    pick = slice(None) if c.pick is None else list(c.pick)
    ref = copy.deepcopy(p.cell).double()
    ref.sigma = _tanh
    X, h0 = p.X[pick].double(), p.h0[pick].double()
    train = c.mode == 'train'
    X.requires_grad_(train and c.dx)
    h0.requires_grad_(train and c.dh0)
    head = None if p.head is None else [t.double().requires_grad_(train) for t in p.head]
    with torch.enable_grad() if train else torch.no_grad():
        H = ref(X, h0)
        assert H.dtype == torch.float64
        key = (c.path, c.gating, c.graph, c.N)
        if key not in _PINNED:
            _shape_sweep().pin_cell_to_torch_reference(ref, np.array(p.S), X.detach(), h0.detach(), H.detach())
            _PINNED.add(key)
        res = {}
        if c.kind == 'native':
            ref2 = copy.deepcopy(p.cell2).double()
            ref2.sigma = _tanh
            res['H1'] = H
            H = ref2(H, h0)
            out, name = H, 'H'
        elif head is not None:
            out, name = _apply_head(c, H, head), 'y'
        else:
            out, name = (H[:, -1:] if c.last_only else H), 'H'
        res[name] = out.detach()
        if train:
            (out * p.dOut[pick].double()).sum().backward()
            res.update(_grads_of(p, ref, head, X, h0, c))
    return {k: v.detach().cpu() for k, v in res.items()}, pick


# ------------------------------------------------------------------------------------------------------------------ bounds
def _assert_h(c, name, got, ref, mx, mn):
    e = (got.double() - ref).abs()
    print('%s %s: max %.3e mean %.3e (bounds %.1e / %.1e)' % (c.id, name, float(e.max()), float(e.mean()), mx, mn))
    assert float(e.max()) <= mx and float(e.mean()) <= mn, (c.id, name, float(e.max()), float(e.mean()), mx, mn)


def _check_bf16(c, got, ref):
    """The bf16 kernels at the bounds of tests/test_directed_uniform.py / tests/test_wide.py (_h_bounds) and the class gates of the bf16
    gradients (GRAD_MAX / GRAD_MEAN through _grad_scale_and_bounds; a scalar bias on its sibling weight's scale), as _train_and_check does."""
    from test_directed_uniform import _h_bounds
    from test_fused import _grad_scale_and_bounds
    from test_gate_extremes import GRAD_MAX, GRAD_MEAN
    mx, mn = _h_bounds(types.SimpleNamespace(sg=c.sg, G=c.G, tg=c.tg))
    if c.shape == 'G1' and c.sg == 'node':
        mx, mn = 6.0e-2, 3.0e-3                                 # (tests/test_wide.py, the node-gated passes at G = 1: one input tap of +-0.45 per hop)
    for name in ('H', 'H1'):
        if name in ref:
            _assert_h(c, name, got[name], ref[name], mx, mn)
    if 'y' in ref:                                              # the head: ||w||_1 times the bound on H (tests/test_directed_uniform.py)
        from test_directed_uniform import _head_weights
        tol = float(np.abs(_head_weights(c.F)).sum()) * mx
        if got['y'].dtype == torch.bfloat16:                    # the training head stores y in bf16: half an ulp, 2^-9 of |y|
            tol += 2.0 ** -9 * float(ref['y'].abs().max())
        _assert_h(c, 'y', got['y'], ref['y'], tol, tol)
    grads = {k[5:]: v.numpy() for k, v in ref.items() if k.startswith('grad:')}
    pgrads = {k: v for k, v in grads.items() if k not in ('X', 'h0')}
    missed = []
    for k, gr in grads.items():
        assert 'grad:' + k in got, (c.id, k, sorted(got))
        e = np.abs(got['grad:' + k].double().numpy() - gr)
        sc, tmax, tmean = float(np.abs(gr).max()), GRAD_MAX, GRAD_MEAN
        if sc == 0.0:                                           # (the unused output gate)
            assert float(e.max()) == 0.0, k
            continue
        if gr.size == 1 and k.endswith('.bias'):
            sc = max(sc, float(np.abs(grads.get(k[:-5] + '.weight', gr)).max()))
        elif k not in ('X', 'h0'):
            sc, tmax, tmean = _grad_scale_and_bounds(k, pgrads, GRAD_MAX, GRAD_MEAN)
        ok = e.max() <= tmax * sc and (e.size < 16 or e.mean() <= tmean * sc)
        print('%s grad %s: max %.3e mean %.3e of its max (bounds %.1e / %.1e)%s' % (c.id, k, e.max() / sc, e.mean() / sc, tmax, tmean, '' if ok else '  MISSED'))
        if not ok:
            missed.append((k, e.max() / sc, e.mean() / sc))
    assert not missed, (c.id, missed)
    for k in got:
        if k.startswith('grad:') and k not in ref:
            assert float(got[k].double().abs().max()) == 0.0, (c.id, k)


def _check_rel(c, got, ref, htol, gtol):
    """States within htol, every gradient within gtol of its own maximum: the x3 kernels (1e-5 / 2e-5), the small-graph kernels
    (1e-11 / 1e-9 in fp64, 1e-5 / 5e-4 in fp32), the composed fp64 path (1e-11 / 1e-10)."""
    for name in ('H', 'y'):
        if name in ref:
            _assert_h(c, name, got[name], ref[name], htol, htol)
    for k, gr in ref.items():
        if not k.startswith('grad:'):
            continue
        assert k in got, (c.id, k, sorted(got))
        sc = float(gr.abs().max())
        e = float((got[k].double() - gr).abs().max())
        if sc == 0.0:
            assert e == 0.0, k
            continue
        print('%s %s: %.3e of its max (bound %.1e)' % (c.id, k, e / sc, gtol))
        assert e <= gtol * sc, (c.id, k, e / sc, gtol)
    for k in got:
        if k.startswith('grad:') and k not in ref:
            assert float(got[k].double().abs().max()) == 0.0, (c.id, k)


def _check(c, got, ref):
    if c.bounds is not None:
        if c.bounds[0] == 'abs':                                # the streaming bf16 path: 5e-2 max, 4e-3 mean
            return _assert_h(c, 'H', got['H'], ref['H'], c.bounds[1], c.bounds[2])
        return _check_rel(c, got, ref, *c.bounds)
    return _check_bf16(c, got, ref)


# ------------------------------------------------------------------------------------------------------------------ routes
def _ops():
    from gated_gcrnns_amd import ops
    return ops


def _route_fused(c, cell, X, h0):
    """bf16 inference: the predicate of the gating, and -- where a kernel is forced -- the plan queries the suite uses to tell them apart."""
    ops = _ops()
    pred = {None: cell._use_fused, 'node': cell._use_fused_node, 'edge': cell._use_fused_edge}[c.sg]
    if c.shape == 'F20':
        assert cell._state_padded(X, h0) is not None
        return
    assert pred(X, h0), c.id
    if c.kernel is None or c.sg is not None:
        return
    Gp = ops.fused_padded_inputs(c.F, c.G)
    graph = cell.graph
    assert graph.fused_plan_img16() is not None
    plan = ops.fused_wide_plan(graph, c.B, c.T, c.N, c.F, Gp, c.K, not c.tg)
    if c.kernel in ('wide', 'hop'):
        assert plan is not None, c.id
        if c.tg:
            assert ops.fused_gate_pair_plan(graph, c.B, c.T, c.N, c.F, Gp, c.K, True)[0] is not None
        scratch = ops.fused_state_scratch(plan, c.B, c.F, X.device)
        want_scratch = c.env.get('GCRNN_SEQ32_STATE_SCRATCH') != '0' and c.kernel == 'wide'
        assert (scratch is not None) == want_scratch, (c.id, scratch is not None)
        if not c.tg and c.kind in ('cell', 'head'):
            user = ops.fused_wide_user_plan(graph, X, h0, c.F, c.G, c.K, head=(c.kind == 'head'))
            want_user = want_scratch and c.env.get('GCRNN_SEQ32_SELF_START') != '0' and not c.env.get('GCRNN_NO_INLINE_PACK')
            assert (user is not None) == want_user, (c.id, user is not None)
    else:
        assert plan is None, c.id
    if c.kind == 'head':
        assert ops.fused_wide_head_supported(graph, c.B, c.T, c.N, c.F, Gp, c.K, c.tg)


def _route_fused_train(c, cell, X, h0):
    from gated_gcrnns_amd import _lib
    ops = _ops()
    assert cell._use_fused_training(X, h0), c.id
    pa = cell.graph.fused_plan_img16(adjoint=True)
    assert pa is not None
    inline = 1 if ops.fused_inline_pack_ok(cell.graph.fused_plan(adjoint=True), c.N, c.F, c.F, c.K) else 0
    assert _lib.lib.gcrnn_fused_backward_data_wide_supported(c.B, c.T, c.N, c.F, c.K, int(pa['entries']), float(pa['uniform_w']), 1, inline) == 1
    assert bool(os.environ.get('GCRNN_NO_WIDE_CHAIN')) == (c.kernel == 'step')
    if c.kind == 'train_head':
        assert ops.fused_cell_head_train_supported(cell.graph, c.B, c.T, c.N, c.F, c.K, torch.float32)


def _route_native(c, cell, X, h0):
    assert _ops().fused_supported(c.N, c.F, c.G, c.Kin, c.Kst, torch.bfloat16, 1) and cell.graph.fused_plan()['npad'] > c.N


def _route_x3(c, cell, X, h0):
    if c.mode == 'train':
        assert cell._use_fused_x3_training(X, h0, time_gated=c.tg), c.id
        return
    if c.sg == 'node':
        assert cell._use_fused_x3_node(X, h0), c.id
    elif c.sg == 'edge':
        assert cell._use_fused_x3_edge(X, h0), c.id
    else:
        assert cell._use_fused_x3(X, h0, time_gated=c.tg), c.id
    if c.graph == 'rank1':
        assert cell.graph.fused_plan_x3().get('rank1_x3') is not None


def _route_horner(c, cell, X, h0):
    assert cell._use_horner(X, h0) and not cell._use_fused(X, h0) and not cell._use_small(X, h0), c.id
    assert not cell._use_fused_x3(X, h0, time_gated=c.tg)


def _route_composed(c, cell, X, h0):
    taken = [n for n in ('_use_fused_training', '_use_fused', '_use_fused_node', '_use_fused_edge', '_use_small', '_use_small_training',
                         '_use_small_edge', '_use_small_edge_training', '_use_horner') if getattr(cell, n)(X, h0)]
    assert not taken and not cell._use_fused_x3_training(X, h0) and cell._state_padded(X, h0) is None, (c.id, taken)


def _route_small(c, cell, X, h0):
    ops = _ops()
    train = c.mode == 'train'
    gated = c.tg or c.sg is not None
    if c.sg == 'edge':
        assert (cell._use_small_edge_training if train else cell._use_small_edge)(X, h0), c.id
        assert bool(os.environ.get('GCRNN_SMALL_EDGE_DX')) == c.dx
        return
    assert (cell._use_small_training if train else cell._use_small)(X, h0), c.id
    dense = ops.small_dense_supported(c.N, c.G, c.F, c.Kin, c.Kst, X.dtype, backward=train, gated=gated)
    assert dense == (c.family == 'mfma'), (c.id, dense)
    if c.kind in ('classify', 'regress'):
        q = ops.small_head_supported if c.kind == 'classify' else ops.small_node_head_supported
        assert q(c.N, c.G, c.F, c.Kin, c.Kst, c.O, X.dtype, train, gated, dx=train and c.dx), c.id


# ------------------------------------------------------------------------------------------------------------------ the cases
def _cases():
    from test_directed_uniform import FORWARD_ENV
    from test_gate_extremes import CHAIN_ENV
    out = []

    def add(id, *a, **k):
        out.append(Case(id, *a, **k))
    small_batch = {'GCRNN_SEQ32_MIN_B': '1'}
    # ---- bf16 fused inference: every kernel, U400 and U1000, un-gated and time-gated (the hop kernel has no gated variant)
    for shape in ('U400', 'U1000'):
        for kernel in ('wide', 'hop', 'seq16', 'step'):
            for gating in ('none', 'time'):
                if kernel == 'hop' and gating == 'time':
                    continue
                add('fused-%s-%s-%s' % (kernel, gating, shape), 'fused', shape, gating, env=FORWARD_ENV[kernel], kernel=kernel, route=_route_fused)
                add('fused-%s-%s-%s-nopack' % (kernel, gating, shape), 'fused', shape, gating, env=dict(FORWARD_ENV[kernel], GCRNN_NO_INLINE_PACK='1'),
                    kernel=kernel, route=_route_fused)
        for gating in ('none', 'time'):
            wide = FORWARD_ENV['wide']
            add('fused-wide-%s-%s-noscratch' % (gating, shape), 'fused', shape, gating, env=dict(wide, GCRNN_SEQ32_STATE_SCRATCH='0'), kernel='wide', route=_route_fused)
            add('fused-wide-%s-%s-scratch' % (gating, shape), 'fused', shape, gating, env=dict(wide, GCRNN_SEQ32_STATE_SCRATCH='1'), kernel='wide', route=_route_fused)
            add('fused-wide-%s-%s-last' % (gating, shape), 'fused', shape, gating, env=wide, kernel='wide', route=_route_fused, last_only=True)
            add('fused-step-%s-%s-last' % (gating, shape), 'fused', shape, gating, env=FORWARD_ENV['step'], kernel='step', route=_route_fused, last_only=True)
            add('fused-head-%s-%s' % (gating, shape), 'fused', shape, gating, env=wide, kernel='wide', route=_route_fused, kind='head')
        add('fused-wide-none-%s-noselfstart' % shape, 'fused', shape, 'none', env=dict(FORWARD_ENV['wide'], GCRNN_SEQ32_SELF_START='0'), kernel='wide', route=_route_fused)
        add('fused-wide-none-%s-selfstart' % shape, 'fused', shape, 'none', env=dict(FORWARD_ENV['wide'], GCRNN_SEQ32_SELF_START='1'), kernel='wide', route=_route_fused)
        add('fused-wide-none-%s-noselfstart-last' % shape, 'fused', shape, 'none', env=dict(FORWARD_ENV['wide'], GCRNN_SEQ32_SELF_START='0'), kernel='wide',
            route=_route_fused, last_only=True)
        add('fused-wide-none-%s-hzero' % shape, 'fused', shape, 'none', env=FORWARD_ENV['wide'], kernel='wide', route=_route_fused, hz=True)
        add('fused-head-none-%s-selfstart' % shape, 'fused', shape, 'none', env=FORWARD_ENV['wide'], kernel='wide', route=_route_fused, kind='head', self_start=True)
        add('fused-head-none-%s-noselfstart' % shape, 'fused', shape, 'none', env=dict(FORWARD_ENV['wide'], GCRNN_SEQ32_SELF_START='0'), kernel='wide',
            route=_route_fused, kind='head')
        for gating in ('node', 'time+node', 'edge'):              # the spatially gated cells: the wide kernel's passes and the 16-feature ones
            add('fused-wide-%s-%s' % (gating, shape), 'fused', shape, gating, env=small_batch, route=_route_fused)
            add('fused-wide-%s-%s-nopack' % (gating, shape), 'fused', shape, gating, env=dict(small_batch, GCRNN_NO_INLINE_PACK='1'), route=_route_fused)
            add('fused-seq16-%s-%s' % (gating, shape), 'fused', shape, gating, env=FORWARD_ENV['seq16'], route=_route_fused)
            add('fused-wide-%s-%s-last' % (gating, shape), 'fused', shape, gating, env=small_batch, route=_route_fused, last_only=True)
    # ---- the four other shapes on the default dispatch (small batches on the persistent kernels)
    for shape in ('U1008', 'U204', 'G1', 'F20'):
        for gating in GATINGS:
            if gating == 'edge' and shape in ('F20', 'U204'):
                continue                                        # (_state_padded: un-gated, time-gated and node-gated cells; the edge-gated passes: N % 8 == 0)
            add('fused-default-%s-%s' % (gating, shape), 'fused', shape, gating, env=small_batch, route=_route_fused,
                pick=(0, 129, 259) if shape == 'U1008' else None)
    # ---- all three graph weightings on U1000 (uniform: above)
    for graph in ('rank1', 'weighted'):
        for gating in GATINGS:
            add('fused-default-%s-U1000-%s' % (gating, graph), 'fused', 'U1000', gating, graph=graph, env=small_batch, route=_route_fused)
    # ---- bf16 fused training: both chains, every gating, dX / dh0 where the fused path hands them out (un-gated and time-gated, G == F)
    for shape in ('U400', 'U1000'):
        for chain in ('wide', 'step'):
            for gating in GATINGS:
                sg = GATINGS[gating][1]
                add('train-%s-%s-%s' % (chain, gating, shape), 'train', shape, gating, prec='master', mode='train', env=CHAIN_ENV[chain], kernel=chain,
                    route=_route_fused_train, dx=sg is None, dh0=sg is None)
            add('train-%s-none-%s-nopack' % (chain, shape), 'train', shape, 'none', prec='master', mode='train', env=dict(CHAIN_ENV[chain], GCRNN_NO_INLINE_PACK='1'),
                kernel=chain, route=_route_fused_train, dx=True, dh0=True)
        for gating in ('none', 'time'):
            add('train-head-%s-%s' % (gating, shape), 'train', shape, gating, prec='master', mode='train', env=CHAIN_ENV['wide'], kernel='wide',
                route=_route_fused_train, kind='train_head', dx=True, dh0=True)
    # ---- two stacked native-layout cells
    for gating in ('none', 'time'):
        add('native-stack-%s-U1000' % gating, 'native', 'U1000', gating, env=small_batch, route=_route_native, kind='native')
    # ---- fp32-accurate x3 kernels: forward for none, time, node, edge; training for none and time; zero and non-zero h0; uniform and rank-1
    x3 = (1e-5, 2e-5)
    for shape in ('X400', 'X1000'):
        for gating in ('none', 'time', 'node', 'edge'):
            for hz in (False, True):
                add('x3-fwd-%s-%s%s' % (gating, shape, '-hzero' if hz else ''), 'x3', shape, gating, prec='f32', route=_route_x3, bounds=x3, hz=hz)
        for gating in ('none', 'time'):
            for hz in (False, True):
                add('x3-train-%s-%s%s' % (gating, shape, '-hzero' if hz else ''), 'x3', shape, gating, prec='f32', mode='train', route=_route_x3, bounds=x3, hz=hz,
                    dh0=(gating == 'none'))
        add('x3-fwd-none-%s-rank1' % shape, 'x3', shape, 'none', graph='rank1', prec='f32', route=_route_x3, bounds=x3)
        add('x3-fwd-time-%s-rank1' % shape, 'x3', shape, 'time', graph='rank1', prec='f32', route=_route_x3, bounds=x3, hz=True)
        add('x3-train-none-%s-rank1' % shape, 'x3', shape, 'none', graph='rank1', prec='f32', mode='train', route=_route_x3, bounds=x3, dh0=True)
    # ---- streaming (Horner form) beyond the LDS-resident kernels
    add('stream-f32-none-S1500', 'stream', 'S1500', 'none', prec='f32', route=_route_horner, bounds=(1e-5, None))
    add('stream-f32-time-S1500', 'stream', 'S1500', 'time', prec='f32', route=_route_horner, bounds=(1e-5, None))
    add('stream-bf16-none-S1500', 'stream', 'S1500', 'none', prec='bf16', route=_route_horner, bounds=('abs', 5e-2, 4e-3))
    # ---- composed fp64 training at the g3_cell_* shape, every gating
    g3 = dict(N=30, F=5, G=2, Kin=3, Kst=3, B=3, T=4)
    for gating in GATINGS:
        add('composed-f64-%s-g3' % gating, 'composed', 'g3', gating, graph='g3', prec='f64', mode='train', route=_route_composed, bounds=(1e-11, 1e-10),
            dims=g3, sigma=_tanh, dx=True, dh0=True)
    # ---- small-graph kernels: both families, both precisions, forward and training with dX
    small = {torch.float64: (1e-11, 1e-9), torch.float32: (1e-5, 5e-4)}
    graphs = {'adj59': dict(N=59, F=20, G=1, Kin=4, Kst=4, B=3, T=4), 'dir17': dict(N=17, F=7, G=3, Kin=3, Kst=2, B=3, T=3)}
    for gname, dims in graphs.items():
        for prec, dt in (('f32', torch.float32), ('f64', torch.float64)):
            for family in ('mfma', 'gather'):
                env = {'GCRNN_SMALL_GATHER': '1'} if family == 'gather' else {}
                for gating in ('none', 'time', 'node'):
                    if gating == 'node' and family == 'gather':
                        continue                                # (per-node gates: the matrix-core family only)
                    for mode in ('infer', 'train'):
                        add('small-%s-%s-%s-%s-%s' % (family, prec, gating, 'fwd' if mode == 'infer' else 'train', gname), 'small', gname, gating, graph=gname,
                            prec=prec, mode=mode, env=env, route=_route_small, bounds=small[dt], dims=dims, family=family, dx=mode == 'train', dh0=mode == 'train')
            add('small-edge-%s-fwd-%s' % (prec, gname), 'small', gname, 'edge', graph=gname, prec=prec, route=_route_small, bounds=small[dt], dims=dims)
            add('small-edge-%s-train-%s' % (prec, gname), 'small', gname, 'edge', graph=gname, prec=prec, mode='train', route=_route_small, bounds=small[dt],
                dims=dims, dh0=True)
            add('small-edge-%s-train-dx-%s' % (prec, gname), 'small', gname, 'edge', graph=gname, prec=prec, mode='train', env={'GCRNN_SMALL_EDGE_DX': '1'},
                route=_route_small, bounds=small[dt], dims=dims, dx=True, dh0=True)
            for kind, O in (('classify', 11), ('regress', 2)):
                for gating in ('none', 'time'):
                    for mode in ('infer', 'train'):
                        add('small-%s-%s-%s-%s-%s' % (kind, prec, gating, 'fwd' if mode == 'infer' else 'train', gname), 'small', gname, gating, graph=gname,
                            prec=prec, mode=mode, route=_route_small, bounds=small[dt], dims=dims, family='mfma', kind=kind, O=O, dx=mode == 'train',
                            dh0=mode == 'train')
    return out


CASES = _cases()
_ENV_KEYS = ('GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ32P', 'GCRNN_SEQ32', 'GCRNN_SEQ_MIN_B', 'GCRNN_SEQ_KERNEL', 'GCRNN_NO_INLINE_PACK', 'GCRNN_NO_WIDE_CHAIN',
             'GCRNN_SEQ32_NODE', 'GCRNN_SEQ32_STATE_SCRATCH', 'GCRNN_SEQ32_SELF_START', 'GCRNN_SMALL_GATHER', 'GCRNN_SMALL_EDGE_DX', 'GCRNN_NO_SMALL_EDGE',
             'GCRNN_NO_SMALL_HEAD', 'GCRNN_NO_SMALL_NODE_HEAD', 'GCRNN_NO_HEAD_CHAIN', 'GCRNN_NO_WIDE_HEAD', 'GCRNN_NO_IMG16', 'GCRNN_NO_GATE_PAIR',
             'GCRNN_NO_X3_GATED', 'GCRNN_NO_X3_EDGE', 'GCRNN_NO_X3_TRAINING', 'GCRNN_NO_X3_NODE', 'GCRNN_FUSED_OVERLAP', 'GCRNN_NO_RANK1', 'GCRNN_NO_UNIFORM')


def _set_env(monkeypatch, env):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_case_table_covers_the_paths_and_switches():
    """CPU: every row of the coverage table is present for every gating it supports, every value of every switch appears, ids are unique."""
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    by = lambda **kw: [c for c in CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for shape in ('U400', 'U1000'):
        for kernel in ('wide', 'hop', 'seq16', 'step'):
            assert by(path='fused', shape=shape, kernel=kernel)
        for gating in GATINGS:
            assert by(path='fused', shape=shape, gating=gating) and by(path='fused', shape=shape, gating=gating, last_only=True)
            for chain in ('wide', 'step'):
                assert by(path='train', shape=shape, gating=gating, kernel=chain)
        for key, values in (('GCRNN_SEQ32_STATE_SCRATCH', ('0', '1')), ('GCRNN_SEQ32_SELF_START', ('0', '1')), ('GCRNN_NO_INLINE_PACK', ('1', None))):
            for v in values:
                assert [c for c in by(path='fused', shape=shape) if c.env.get(key) == v], (shape, key, v)
        assert by(shape=shape, kind='head', self_start=True) and by(shape=shape, kind='head', self_start=False) and by(shape=shape, kind='train_head')
    for shape in ('U1008', 'U204', 'G1', 'F20'):
        assert len(by(path='fused', shape=shape)) >= 4
    for graph in ('uniform', 'rank1', 'weighted'):
        assert len(by(path='fused', shape='U1000', graph=graph)) >= 5
    assert len(by(kind='native')) == 2
    for shape in ('X400', 'X1000'):
        for graph in ('uniform', 'rank1'):
            assert by(path='x3', shape=shape, graph=graph, mode='infer') and by(path='x3', shape=shape, graph=graph, mode='train')
        for hz in (False, True):
            assert by(path='x3', shape=shape, hz=hz, mode='infer') and by(path='x3', shape=shape, hz=hz, mode='train')
    assert len(by(path='stream')) == 3 and len(by(path='composed')) == 5
    for gname in ('adj59', 'dir17'):
        for prec in ('f32', 'f64'):
            for family in ('mfma', 'gather'):
                assert by(path='small', graph=gname, prec=prec, family=family, mode='infer') and by(path='small', graph=gname, prec=prec, family=family, mode='train')
            assert len(by(path='small', graph=gname, prec=prec, gating='edge')) == 3
            assert by(graph=gname, prec=prec, kind='classify') and by(graph=gname, prec=prec, kind='regress')
    for v in ('1', None):
        assert [c for c in CASES if c.env.get('GCRNN_SMALL_GATHER') == v] and [c for c in CASES if c.env.get('GCRNN_SMALL_EDGE_DX') == v]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_path_is_independent_of_its_workspace(case, monkeypatch):
    c = case
    _set_env(monkeypatch, c.env)
    runs = assert_independent_of_workspace(lambda: _run_kernels(c))
    ref, pick = _run_reference(c)
    got = runs['zero']
    if c.pick is not None:                                      # (the fp64 run takes a few of the sequences; inference only: gradients sum over all)
        assert c.mode == 'infer'
        got = {k: v[pick] for k, v in got.items()}
    _check(c, got, ref)


# ================================================================================================================== GPU: stand-alone ops
def _rel_check(tag, got, ref, tol, floor=0.0, absolute=()):
    """|got - ref| <= tol * max(floor, max|ref|), name by name (the names in `absolute`: <= tol)."""
    for k, r in ref.items():
        assert k in got, (tag, k, sorted(got))
        r = r.detach().double().cpu()
        sc = 1.0 if k in absolute else max(floor, float(r.abs().max()))
        e = float((got[k].double() - r).abs().max())
        t = tol[k] if isinstance(tol, dict) else tol
        print('%s %s: %.3e of %.3e (bound %.1e)' % (tag, k, e, sc, t))
        assert e <= t * sc + 1e-300, (tag, k, e / max(sc, 1e-300), t)


def _edit(edit, **operands):
    """run(edit=...) of the makers below: edit({name: device operand}) may write into the operands before the op runs (the data operands
    only; tests/test_sequence_isolation.py puts one non-finite element there). Without it the operands are the seeded ones."""
    if edit is not None:
        with torch.no_grad():
            edit(operands)


def _op_graph_filter_layer(Fin, Fout, K, prec):
    """graph_filter_layer forward and backward at N = 59 (the epicenter graph): taps-first (F_out < F_in) and hops-first, at the bounds of
    tests/test_gnn_heads.py: bf16 x with fp32 parameters 1e-4 (dx, stored in bf16: 1e-2), fp32 1e-5, fp64 1e-11, of max(1, max|ref|)."""
    from conftest import GOLDEN
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator
    xdt, wdt = {'bf16': (torch.bfloat16, torch.float32), 'f32': (torch.float32,) * 2, 'f64': (torch.float64,) * 2}[prec]
    S = np.load(os.path.join(GOLDEN, 'adj59.npy')).reshape(1, 59, 59)
    S = S / np.max(np.abs(np.linalg.eigvals(S[0])))
    N, items = 59, 5

    def operands():
        g = torch.Generator().manual_seed(Fin * 10 + Fout + K)
        x = torch.randn(items, Fin, N, generator=g, dtype=torch.float64).to(xdt)
        w = (torch.rand(Fout, 1, K, Fin, generator=g, dtype=torch.float64) * 2 - 1).div(np.sqrt(Fin * K)).to(wdt)
        b = (torch.rand(Fout, 1, generator=g, dtype=torch.float64) - 0.5).to(wdt)
        dy = torch.randn(items, Fout, N, generator=g, dtype=torch.float64).to(wdt)
        return x, w, b, dy

    def run(edit=None):
        graph = GraphOperator(S, device=DEV)
        assert ops.graph_filter_layer_supported(xdt, wdt, graph, Fin, Fout, K)
        x, w, b, dy = (t.to(DEV) for t in operands())
        _edit(edit, x=x)
        for t in (x, w, b):
            t.requires_grad_(True)
        y = ops.graph_filter_layer(x, w, b, graph, 'tanh')
        y.backward(dy)
        return {'y': y.detach(), 'dx': x.grad, 'dw': w.grad, 'db': b.grad}

    def check(got):
        x, w, b, dy = (t.double().to(DEV).requires_grad_(i < 3) for i, t in enumerate(operands()))
        Sd = torch.tensor(S[0], dtype=torch.float64, device=DEV)
        z, acc = x, 0.0
        for k in range(K):
            acc = acc + torch.einsum('fg,ign->ifn', w[:, 0, k], z)
            z = z @ Sd
        y = torch.tanh(acc + b.view(1, Fout, 1))
        y.backward(dy)
        tol = {'bf16': 1e-4, 'f32': 1e-5, 'f64': 1e-11}[prec]
        _rel_check('gfl', got, {'y': y, 'dx': x.grad, 'dw': w.grad, 'db': b.grad}, {'y': tol, 'dx': 1e-2 if prec == 'bf16' else tol, 'dw': tol, 'db': tol}, 1.0)
    return run, check


def _op_node_linear(R, F, N, O, prec):
    """node_linear forward and backward (tests/test_hip_parity.py): fp32 to 2e-5 of each result's max; bf16 activations and weights to bf16
    rounding (y 2^-8, gradients 2^-7) of the fp64 result on the same bf16 values."""
    from gated_gcrnns_amd import ops
    dt = torch.float32 if prec == 'f32' else torch.bfloat16

    def operands():
        g = torch.Generator().manual_seed(R + N)
        # dy = 0.5 + N(0, 1): db = sum of R N terms is a scalar at O = 1, and a sum that cancels is no scale for its own rounding error
        return (torch.randn(R, F, N, generator=g).to(dt), (torch.randn(O, F, generator=g) / F ** 0.5).to(dt), torch.randn(O, generator=g).to(dt),
                (0.5 + torch.randn(R, O, N, generator=g)).to(dt))

    def run(edit=None):
        assert ops.node_linear_supported(F, O, dt, N, dt)
        h, w, b, dy = (t.to(DEV) for t in operands())
        _edit(edit, h=h)
        for t in (h, w, b):
            t.requires_grad_(True)
        y = ops.node_linear(h, w, b)
        (y.float() * dy.float()).sum().backward()
        return {'y': y.detach(), 'dh': h.grad, 'dw': w.grad, 'db': b.grad}

    def check(got):
        h, w, b, dy = (t.double().to(DEV).requires_grad_(i < 3) for i, t in enumerate(operands()))
        y = torch.nn.functional.linear(h.transpose(1, 2), w, b).transpose(1, 2)
        (y * dy).sum().backward()
        tol = 2e-5 if prec == 'f32' else {'y': 2.0 ** -8, 'dh': 2.0 ** -7, 'dw': 2.0 ** -7, 'db': 2.0 ** -7}
        _rel_check('node_linear', got, {'y': y, 'dh': h.grad, 'dw': w.grad, 'db': b.grad}, tol)
    return run, check


def _op_rnn_sequence(B, T, D, Fh, bias, prec):
    """rnn_sequence forward and backward against the plain-torch fp64 recurrence of tests/test_rnn_baseline.py: 1e-5 (fp32), 1e-11 (fp64)."""
    from gated_gcrnns_amd import ops
    dt = {'f32': torch.float32, 'f64': torch.float64}[prec]
    names = ('x', 'h0', 'w_ih', 'w_hh', 'b_ih', 'b_hh')

    def run(edit=None):
        from test_rnn_baseline import _case
        assert ops.rnn_supported(dt, B, T, D, Fh)
        ts, ks, Rr = _case(B, T, D, Fh, 'tanh', bias, dt, seed=B * 1000 + T * 10 + Fh)
        _edit(edit, x=ks[0], h0=ks[1])
        H = ops.rnn_sequence(*ks, 'tanh')
        (H * Rr.to(dt)).sum().backward()
        out = {'H': H.detach()}
        out.update({'d' + n: k.grad for n, k in zip(names, ks) if k is not None})
        return out

    def check(got):
        from test_rnn_baseline import _case, torch_rnn
        ts, ks, Rr = _case(B, T, D, Fh, 'tanh', bias, dt, seed=B * 1000 + T * 10 + Fh)
        ref = torch_rnn(*ts, 'tanh')
        (ref * Rr).sum().backward()
        want = {'H': ref}
        want.update({'d' + n: t.grad for n, t in zip(names, ts) if t is not None})
        _rel_check('rnn', got, want, {'f32': 1e-5, 'f64': 1e-11}[prec])
    return run, check


def _op_l1_loss(shape, prec):
    """l1_loss with backward (tests/test_hip_parity.py test_l1_loss_kernel): ties, an upstream gradient of 3, its tolerances."""
    from gated_gcrnns_amd import ops
    dt, tol = {'f64': (torch.float64, 1e-13), 'f32': (torch.float32, 1e-6), 'bf16': (torch.bfloat16, 2e-3)}[prec]

    def operands():
        g = torch.Generator().manual_seed(5)
        x = torch.randn(*shape, generator=g, dtype=torch.float64).to(dt)
        y = torch.randn(*shape, generator=g, dtype=torch.float64).to(dt)
        y.view(-1)[::7] = x.view(-1)[::7]
        return x, y

    def run(edit=None):
        x, y = (t.to(DEV).requires_grad_(True) for t in operands())
        _edit(edit, x=x)
        loss = ops.l1_loss(x, y)
        (3.0 * loss).backward()
        return {'loss': loss.detach(), 'dx': x.grad, 'dy': y.grad}

    def check(got):
        x, y = (t.double().requires_grad_(True) for t in operands())
        ref = torch.nn.functional.l1_loss(x, y)
        (3.0 * ref).backward()
        n = x.numel()
        assert abs(float(got['loss']) - float(ref)) <= tol * max(1.0, abs(float(ref)))
        gtol = tol * 3.0 / n + (1e-2 * 3.0 / n if dt == torch.bfloat16 else 0)
        assert float((got['dx'].double() - x.grad).abs().max()) <= gtol and float((got['dy'].double() - y.grad).abs().max()) <= gtol
    return run, check


def _op_batch_time_mse(prec):
    """batch_time_mse on [65][1000] (tests/test_hip_parity.py: 1e-12 fp64, 1e-5 fp32 and bf16, relative)."""
    from gated_gcrnns_amd import ops
    dt, tol = {'f64': (torch.float64, 1e-12), 'f32': (torch.float32, 1e-5), 'bf16': (torch.bfloat16, 1e-5)}[prec]

    def operands():
        g = torch.Generator().manual_seed(13)
        return torch.randn(65, 1000, generator=g, dtype=torch.float64).to(dt), torch.randn(65, 1000, generator=g, dtype=torch.float64).to(dt)

    def run(edit=None):
        x, y = (t.to(DEV) for t in operands())
        _edit(edit, x=x)
        return {'metric': ops.batch_time_mse(x, y)}

    def check(got):
        xv, yv = (t.double() for t in operands())
        want = torch.mean(torch.sqrt(torch.sum((xv - yv) ** 2, dim=0)) / torch.norm(yv, dim=0))
        assert abs(float(got['metric']) - float(want)) <= tol * float(want), (float(got['metric']), float(want))
    return run, check


def _op_cross_entropy(B, C, tag):
    """cross_entropy with hits against fp64 on the host (tests/test_cross_entropy.py, its _check)."""
    from gated_gcrnns_amd import ops

    def run(edit=None):
        from test_cross_entropy import DTYPES, _problem
        z, lab = _problem(B, C, DTYPES[tag], 100 * B + C)
        zd = z.to(DEV).requires_grad_(True)
        _edit(edit, z=zd)
        loss, hits = ops.cross_entropy(zd, lab.to(DEV), return_hits=True)
        loss.backward()
        return {'loss': loss.detach(), 'hits': hits, 'dz': zd.grad}

    def check(got):
        from test_cross_entropy import DTYPES, _check, _problem
        z, lab = _problem(B, C, DTYPES[tag], 100 * B + C)
        _check(tag, z, lab, got['loss'], got['dz'], got['hits'])
    return run, check


def _op_edge_attention(prec):
    """edge_attention forward and backward at N = 30, B = 3, F = 5, T = 4 against the index-op restatement of tests/test_hip_parity.py
    (1e-12 fp64, 2e-5 fp32 of each result's max)."""
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator
    dt, tol = {'f64': (torch.float64, 1e-12), 'f32': (torch.float32, 2e-5)}[prec]
    N, B, F, Tn = 30, 3, 5, 4
    rng = np.random.default_rng(N)
    S = rng.standard_normal((N, N)) * (rng.random((N, N)) < 0.1)
    S[3, :] = 0; S[:, 3] = 0
    S[5, 5] = -1.0

    def operands(dtype):
        gen = torch.Generator().manual_seed(0)
        mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(DEV).to(dt).to(dtype)
        return mk(Tn, N, B, F), mk(Tn, N, B), mk(Tn, N, B), mk(Tn, N, B, F)

    def run(edit=None):
        graph = GraphOperator(S[None], device=DEV)
        Wx, s1, s2, r = operands(dt)
        _edit(edit, Wx=Wx)
        for t in (Wx, s1, s2):
            t.requires_grad_(True)
        y = ops.edge_attention(Wx, s1, s2, graph)
        (y * r).sum().backward()
        return {'y': y.detach(), 'dWx': Wx.grad, 'ds1': s1.grad, 'ds2': s2.grad}

    def check(got):
        from test_hip_parity import _attention_torch
        graph = GraphOperator(S[None], device=DEV)
        Wx, s1, s2, r = operands(torch.float64)
        for t in (Wx, s1, s2):
            t.requires_grad_(True)
        y = _attention_torch(Wx, s1, s2, graph)
        (y * r).sum().backward()
        _rel_check('edge_attention', got, {'y': y, 'dWx': Wx.grad, 'ds1': s1.grad, 'ds2': s2.grad}, tol)
    return run, check


def _op_lsigf_two_edge_features(prec):
    """LSIGF with E = 2 edge features (the composed filter ops: node-major pack, one SpMM per hop and feature, the tap kernels) against
    the dense sum in fp64, at the bounds of the g1 fixture test of tests/test_hip_parity.py: y within 1e-11 (fp64) / 1e-5 (fp32), gradients
    within 1e-10 / 2e-5 of their max."""
    import gated_gcrnns_amd.Utils.graphML as gml
    dt, tol, gtol = {'f64': (torch.float64, 1e-11, 1e-10), 'f32': (torch.float32, 1e-5, 2e-5)}[prec]
    N, G, F, K, B, E = 30, 2, 5, 3, 3, 2
    rng = np.random.default_rng(12)
    S = (rng.random((E, N, N)) < 0.15) * rng.uniform(0.2, 1.0, (E, N, N))
    S = S / np.abs(np.linalg.eigvals(S)).max()

    def operands():
        g = torch.Generator().manual_seed(4)
        return (torch.randn(F, E, K, G, generator=g, dtype=torch.float64).div(np.sqrt(G * K * E)).to(dt), torch.randn(B, G, N, generator=g, dtype=torch.float64).to(dt),
                torch.randn(F, 1, generator=g, dtype=torch.float64).to(dt), torch.randn(B, F, N, generator=g, dtype=torch.float64).to(dt))

    def run(edit=None):
        h, x, b, dy = (t.to(DEV) for t in operands())
        _edit(edit, x=x)
        for t in (h, x, b):
            t.requires_grad_(True)
        y = gml.LSIGF(h, torch.tensor(S, dtype=dt, device=DEV), x, b)
        (y * dy).sum().backward()
        return {'y': y.detach(), 'dh': h.grad, 'dx': x.grad, 'db': b.grad}

    def check(got):
        h, x, b, dy = (t.double().to(DEV).requires_grad_(i < 3) for i, t in enumerate(operands()))
        Sd = torch.tensor(S, dtype=torch.float64, device=DEV)
        y = b.view(1, F, 1)
        for e in range(E):
            z = x
            for k in range(K):
                y = y + torch.einsum('fg,bgn->bfn', h[:, e, k], z)
                z = z @ Sd[e]
        (y * dy).sum().backward()
        _rel_check('lsigf', got, {'y': y, 'dh': h.grad, 'dx': x.grad, 'db': b.grad}, {'y': tol, 'dh': gtol, 'dx': gtol, 'db': gtol}, absolute=('y',))
    return run, check


def _op_cases():
    out = []
    for prec in ('bf16', 'f32', 'f64'):
        out.append(('gfl-taps-first-%s' % prec, _op_graph_filter_layer, (20, 1, 4, prec)))
        out.append(('gfl-hops-first-%s' % prec, _op_graph_filter_layer, (20, 21, 4, prec)))
        out.append(('l1-loss-7x1x1x1-%s' % prec, _op_l1_loss, ((7, 1, 1, 1), prec)))
        out.append(('l1-loss-3x4x5x30-%s' % prec, _op_l1_loss, ((3, 4, 5, 30), prec)))
        out.append(('batch-time-mse-%s' % prec, _op_batch_time_mse, (prec,)))
        out.append(('cross-entropy-257x64-%s' % prec, _op_cross_entropy, (257, 64, prec)))
        out.append(('cross-entropy-3x2-%s' % prec, _op_cross_entropy, (3, 2, prec)))
    out.append(('node-linear-40x20x58x1-f32', _op_node_linear, (40, 20, 58, 1, 'f32')))
    out.append(('node-linear-7x64x33x3-f32', _op_node_linear, (7, 64, 33, 3, 'f32')))
    out.append(('node-linear-40x20x58x1-bf16', _op_node_linear, (40, 20, 58, 1, 'bf16')))      # (the bf16 kernels take even N: not 7x64x33x3)
    for prec in ('f32', 'f64'):
        out.append(('rnn-67x3x22x9-nobias-%s' % prec, _op_rnn_sequence, (67, 3, 22, 9, False, prec)))
        out.append(('rnn-5x7x13x1-%s' % prec, _op_rnn_sequence, (5, 7, 13, 1, True, prec)))
        out.append(('edge-attention-%s' % prec, _op_edge_attention, (prec,)))
        out.append(('lsigf-two-edge-features-%s' % prec, _op_lsigf_two_edge_features, (prec,)))
    return out


OPS = _op_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('make,args', [(m, a) for _, m, a in OPS], ids=[i for i, _, _ in OPS])
def test_op_is_independent_of_its_workspace(make, args, monkeypatch):
    _set_env(monkeypatch, {})
    run, check = make(*args)
    runs = assert_independent_of_workspace(run)
    check(runs['zero'])
