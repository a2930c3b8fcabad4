"""A non-finite input stays in its own sequence and step ("A non-finite input stays in its own sequence and step").

The persistent kernels walk several sequences, or (t, b) items, per workgroup with stride gridDim.x; the inline pack lays out the next
step's input -- in the all-items passes the next ITEM's operand -- while the current one is computed; LDS images rest on "padding rows stay
zero" from one item of a workgroup to the next; the weight-gradient kernel carries accumulators and a gate ratio from item to item. Random
finite data hides a stray read there (times zero it is invisible). `0 * NaN` is NaN, so a NaN in ONE sequence at ONE step shows any data
path between sequences or backwards in time as a changed bit somewhere else. Each row builds its problem ONCE (cell, plans, inputs), runs
it clean and then on cloned inputs with one place poisoned, and compares bit for bit on the device (torch.equal) -- no tolerance anywhere.

The contract, at sequence b0, step t0 = 1, channel g0 = 0, node m0 (a node with a neighbour):
  P1  X[b0, t0, g0, m0] = NaN        P2  X[b0, t0, :, :] = NaN        P3  h0[b0, 0, m0] = NaN (not on hz rows)        P4  X[b0, t0, g0, m0] = +Inf
  (I) isolation     every output with a batch axis (H, H1, y, logits, grad:X, grad:h0) is bit-identical to the clean run at b != b0; P1 .. P4
  (C) causality     H[b0, :t0] / y[b0, :t0] is bit-identical to the clean run; P1, P2, P4. Not checkable where the output has no time axis:
                    the `last_only` rows and the classification logits
  (N) no laundering NaN only. P1: H[b0, t >= t0, :, m0] non-finite; P2: H[b0, t0:] non-finite everywhere; P3: H[b0, :, :, m0] non-finite;
                    the same on a per-node head's y; every logit of b0; `last_only`: the same at the last step; training: every element of
                    grad:weight_A (P1, P2) and of grad:weight_B (P3) non-finite. A time-gated cell has ONE scalar gate per (t, b), read
                    from x_t and h0: there P1 is held to P2's statement (all of H[b0, t0:]) and P3 to all of H[b0]
  P4 is held to (I) and (C) only: the sparse kernels give tanh(+-Inf) = +-1 where the dense reference has 0 * Inf = NaN.
test_the_reference_meets_the_contract holds oracle/torch_reference.py (fp64, autograd) to every line on the five g3_cell_* fixtures, so
the contract is a statement about the reference; no line had to be dropped for any gating or pattern. The one exception of DESIGN.md 4.2
(a non-finite operand under a gate at or below its guard is dropped) is not exercised: the gates are at their usual initialisation.

Runs per row: clean; P1 .. P4 at b0 = 1; P2 at b0 = 257; P1 at b0 = 130; for inference the batch reversed (X.flip(0), h0.flip(0) gives
H.flip(0) bit for bit: the batch size, hence the dispatch, is the same). Rows are a predicate over CASES of tests/test_poisoned_workspace.py
with B = 260, T = 3 (small graphs: B = 260 at the table's T; streaming: the table's sizes, so its b0 are 1, B - 1 and B // 2). 256 is
GCRNN_SEQ_MAX_GRID: at B = 260 the workgroup of sequence 1 goes on to sequence 257, and the all-items passes have 780 items on at most 256
workgroups. T = 3 is the smallest T with the inline pack (T > 2) and a step on either side of t0.

Which run reaches which mechanism:
  mechanism                                            | reached by
  second sequence of a workgroup (b -> b + gridDim.x)  | b0 = 1 (is 257, the successor, clean?) and P2 at b0 = 257 (clean predecessor: are
                                                       | images, padding rows and prefetched operands fresh?); P1 at b0 = 130: neither
  next step's input laid out during the current step   | (C): x_1 of b0 is laid out while step 0 runs; `-nopack` rows are the control
  next ITEM's operand laid out by the all-items passes | time / node / edge gated rows: item (t0, b0) is packed by the workgroup's previous
                                                       | item and followed by another; (I) and (C) on every other item
  all-items passes (gate pre-pass, filter output pass, | 780 items on <= 256 workgroups: (I) at b != b0, (C) at (t < t0, b0), (N) at the item
  attention, weight gradient)                          |
  accumulators and gate ratio carried between items    | training rows: grad:X / grad:h0 of b != b0 (I); grad:weight_A / grad:weight_B (N) --
                                                       | a NaN gate must not drop its item from the sum
  batch position                                       | the reversed batch (inference rows)

Findings, 25 of 151 GPU cases before the fixes of the commit that added this file (DESIGN.md 3.2 has the detail):
  1. (N) every edge-gated row (wide, 16-feature, G1, both training chains, the small-graph kernels in fp32 and fp64): the attention layer's
     ReLU was fmaxf(v, 0) / `v > 0 ? v : 0`, which is 0 for a NaN where torch.relu keeps it -- H[b0, t >= t0, :, m0] came out finite. The
     graph-filter layer's and the RNN baseline's ReLU had the same form (test_relu_keeps_a_nan).
  2. (N) every time-gated training row, P3: the weight-gradient kernel's `g > 1e-12f` is false for a NaN gate, so every item of b0 was
     left out of the sum and grad:weight_B was finite. Now `!(g <= 1e-12f)`. The forward guards `g > 1e-30f` did NOT fail: the waves that
     take the tap first multiply by the NaN gate and the hops carry it to every node -- the whole-step lines above pass unchanged.
  3. (R) the reversed batch on the 16-feature node-gated rows and the small-graph rows whose gates come from the composed filter ops: the
     streaming SpMM left `acc += w * x` to the compiler, which fused columns 0, 1 of a lane's four and not columns 2, 3, so a one-channel
     signal's column b and column B - 1 - b were rounded differently. The kernel now says fma for every column.
The stand-alone ops had no finding of their own beyond the two ReLUs.

Wall time of the whole file on the MI355X: 20 s for the 153 GPU cases (0.13 s per case; the slowest, the U1000 training rows, 1.0 s each)."""
import copy
import types

import numpy as np
import pytest
import torch

from test_poisoned_workspace import CASES, OPS, SHAPES, _build, _gso, _run_kernels, _set_env
from test_poisoned_workspace import (_op_batch_time_mse, _op_cross_entropy, _op_edge_attention, _op_graph_filter_layer, _op_l1_loss,
                                     _op_lsigf_two_edge_features, _op_node_linear, _op_rnn_sequence)
from test_poisoned_workspace import (_route_fused, _route_fused_train, _route_horner, _route_native, _route_small, _route_x3)  # noqa: F401  (the rows' routes)

T0, G0 = 1, 0
NAN, INF = float('nan'), float('inf')
BATCH, STEPS = 260, 3
#        pattern, b0 (a b0 the batch does not have: B - 1 for 257, B // 2 for 130)
RUNS = (('P1', 1), ('P2', 1), ('P3', 1), ('P4', 1), ('P2', 257), ('P1', 130))


# ================================================================================================================== the checker
def _runs_for(B):
    out = []
    for pat, b0 in RUNS:
        b0 = b0 if b0 < B else (B - 1 if b0 == 257 else B // 2)
        if (pat, b0) not in out:
            out.append((pat, b0))
    return out


def poison(X, h0, pattern, b0, m0, t0=T0):
    """Clones of the inputs with the pattern written in."""
    X, h0 = X.detach().clone(), h0.detach().clone()
    if pattern == 'P1':
        X[b0, t0, G0, m0] = NAN
    elif pattern == 'P2':
        X[b0, t0] = NAN
    elif pattern == 'P3':
        h0[b0, 0, m0] = NAN
    elif pattern == 'P4':
        X[b0, t0, G0, m0] = INF
    else:
        raise KeyError(pattern)
    return X, h0


def _first(mask):
    idx = torch.nonzero(mask.reshape(mask.shape if mask.dim() else (1,)))
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def _same(line, name, what, got, clean, pattern, b0):
    if got.shape == clean.shape and got.dtype == clean.dtype and torch.equal(got, clean):
        return
    ne = (got != clean) | got.isnan() if got.shape == clean.shape else None
    raise AssertionError('(%s) %s under %s at b0 = %d: output %r %s differs from the clean run, first at index %s of that part (%s of %d elements)' % (
        line, {'I': 'isolation', 'C': 'causality'}[line], pattern, b0, name, what, None if ne is None else _first(ne),
        None if ne is None else int(ne.sum()), got.numel()))


def _nonfinite(name, what, part, pattern, b0):
    assert part.numel() > 0, (name, what)
    fin = torch.isfinite(part)
    if bool(fin.any()):
        raise AssertionError('(N) no laundering under %s at b0 = %d: output %r %s holds finite values, first at index %s of that part (%d of %d elements)' % (
            pattern, b0, name, what, _first(fin), int(fin.sum()), part.numel()))


def layouts_of(c):
    """Output name -> layout. 'bt.n': [B][T][.][N]; 'b1.n': the last state only, [B][1][.][N]; 'b.': [B][.] (logits, no time axis);
    'b': a batch axis and nothing else to state (grad:X, grad:h0). Every other name is a parameter gradient: no batch axis. A trailing
    '!': the cell is time-gated -- one scalar gate per (t, b), so a NaN anywhere in x_t or h0 (the gates read x_t and h0) makes the whole
    step non-finite: P1 and P3 are held to P2's statement (from t0 on, and from step 0 on). The reference has it by construction."""
    whole = '!' if c.tg else ''                                 # (the native stack: the time gates are the second cell's)
    lay = {'grad:X': 'b', 'grad:h0': 'b', 'H1': 'bt.n'}
    lay['H'] = ('b1.n' if c.last_only else 'bt.n') + whole
    lay['y'] = 'b.' if c.kind == 'classify' else 'bt.n' + whole
    return lay


def check_contract(clean, got, pattern, b0, m0, layouts, t0=T0):
    """One poisoned run against the clean one: (I) for every pattern, (C) for P1, P2, P4, (N) for the NaN patterns P1 .. P3."""
    assert got.keys() == clean.keys(), (sorted(got), sorted(clean))
    for name, g in got.items():
        lay = layouts.get(name) if name in layouts or not name.startswith('grad:') else None
        assert lay is not None or name.startswith('grad:'), 'no layout for output %r' % name
        c = clean[name]
        assert g.shape == c.shape and g.dtype == c.dtype, (name, g.shape, c.shape)
        whole = lay is not None and lay.endswith('!')
        lay = lay.rstrip('!') if lay is not None else None
        if lay is None:                                         # a parameter gradient: sums over the batch
            if pattern != 'P4' and name == ('grad:weight_B' if pattern == 'P3' else 'grad:weight_A'):
                _nonfinite(name, '(every element)', g, pattern, b0)
            continue
        _same('I', name, '[:%d]' % b0, g[:b0], c[:b0], pattern, b0)
        _same('I', name, '[%d:]' % (b0 + 1), g[b0 + 1:], c[b0 + 1:], pattern, b0)
        if lay == 'bt.n' and pattern != 'P3':
            _same('C', name, '[%d, :%d]' % (b0, t0), g[b0, :t0], c[b0, :t0], pattern, b0)
        if pattern == 'P4' or lay == 'b':
            continue
        if lay == 'b.':
            _nonfinite(name, '[%d]' % b0, g[b0], pattern, b0)
            continue
        steps = slice(0, None) if lay == 'b1.n' or pattern == 'P3' else slice(t0, None)
        if pattern == 'P2' or whole:
            _nonfinite(name, '[%d, %s:]' % (b0, steps.start), g[b0, steps], pattern, b0)
        else:
            _nonfinite(name, '[%d, %s:, :, %d]' % (b0, steps.start, m0), g[b0, steps, :, m0], pattern, b0)


def assert_contract(run, X, h0, layouts, m0, skip_p3=False, reversal=False):
    """run(X, h0) -> {name: tensor}. One clean run, the poisoned runs of RUNS on clones, and (inference) the reversed batch."""
    B = X.shape[0]
    clean = run(X.detach().clone(), h0.detach().clone())
    for name, t in clean.items():
        assert bool(torch.isfinite(t).all()), 'the clean run is not finite in %r' % name
    done = []
    for pattern, b0 in _runs_for(B):
        if pattern == 'P3' and skip_p3:
            continue
        Xp, hp = poison(X, h0, pattern, b0, m0)
        check_contract(clean, run(Xp, hp), pattern, b0, m0, layouts)
        done.append((pattern, b0))
    if reversal:
        got = run(X.detach().flip(0).contiguous(), h0.detach().flip(0).contiguous())
        for name, t in got.items():
            if not torch.equal(t, clean[name].flip(0)):
                ne = t != clean[name].flip(0)
                raise AssertionError('(R) the reversed batch: output %r is not the clean run reversed, first at index %s (%d of %d elements)' % (
                    name, _first(ne), int(ne.sum()), t.numel()))
    return done


def node_with_a_neighbour(S):
    A = np.array(S).reshape(-1, S.shape[-2], S.shape[-1])[0] != 0
    A = A & ~np.eye(A.shape[0], dtype=bool)
    deg = A.sum(0) + A.sum(1)
    cand = [n for n in range(min(7, A.shape[0] - 1), A.shape[0]) if deg[n] > 0]
    assert cand, 'the graph has no edge'
    return cand[0]


# ================================================================================================================== CPU: the reference
REFERENCE_GATINGS = {'none': (False, None), 'time': (True, None), 'node': (False, 'node'), 'time_node': (True, 'node'), 'edge': (False, 'edge')}


@pytest.mark.parametrize('name', sorted(REFERENCE_GATINGS))
def test_the_reference_meets_the_contract(name):
    """oracle/torch_reference.ggcrnn_cell in fp64 with autograd on the g3_cell_* fixture (B = 3, T = 4, N = 30): every line of the
    contract, the training lines (grad:X, grad:h0, grad:weight_A, grad:weight_B) included, for P1 .. P4 at b0 = 1, P2 at b0 = 2."""
    from conftest import load_golden
    from oracle import torch_reference as tr
    tg, sg = REFERENCE_GATINGS[name]
    g = load_golden('g3_cell_' + name)
    S = torch.tensor(g['S'], dtype=torch.float64)
    dOut = torch.randn(*g['H'].shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)

    def run(X, h0):
        P = {k: torch.tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in g['params'].items()}
        X.requires_grad_(True)
        h0.requires_grad_(True)
        H = tr.ggcrnn_cell(P, S, X, h0, tg, sg)
        (H * dOut).sum().backward()
        return {'H': H.detach(), 'grad:X': X.grad, 'grad:h0': h0.grad, 'grad:weight_A': P['weight_A'].grad, 'grad:weight_B': P['weight_B'].grad}
    lay = {'H': 'bt.n' + ('!' if tg else ''), 'grad:X': 'b', 'grad:h0': 'b'}
    done = assert_contract(run, torch.tensor(g['X'], dtype=torch.float64), torch.tensor(g['h0'], dtype=torch.float64), lay, node_with_a_neighbour(g['S']))
    assert done == [('P1', 1), ('P2', 1), ('P3', 1), ('P4', 1), ('P2', 2)]
    # the last state alone and a read-out over all nodes (the `last_only` and classification lines) are the same statements on H[:, -1]
    w = torch.randn(4, g['H'].shape[2] * g['H'].shape[3], generator=torch.Generator().manual_seed(4), dtype=torch.float64)

    def run_last(X, h0):
        H = tr.ggcrnn_cell({k: torch.tensor(v, dtype=torch.float64) for k, v in g['params'].items()}, S, X, h0, tg, sg)
        return {'H': H[:, -1:], 'y': H[:, -1].reshape(H.shape[0], -1) @ w.t()}
    assert_contract(run_last, torch.tensor(g['X'], dtype=torch.float64), torch.tensor(g['h0'], dtype=torch.float64), {'H': 'b1.n' + ('!' if tg else ''), 'y': 'b.'},
                    node_with_a_neighbour(g['S']))        # (no reversal: a property asked of the kernels; the host BLAS sums by batch position)


# ================================================================================================================== CPU: the checker bites
def _fake_problem():
    B, T, G, F, N = 5, 3, 2, 3, 6
    g = torch.Generator().manual_seed(11)
    return (torch.randn(B, T, G, N, generator=g, dtype=torch.float64), 0.3 * torch.randn(B, F, N, generator=g, dtype=torch.float64),
            torch.randn(F, G, generator=g, dtype=torch.float64), torch.randn(F, F, generator=g, dtype=torch.float64) / 2)


def _fake_kernel(X, h0, W, V, leak=None):
    """h_t = tanh(W x_t + V h_{t-1}) node by node, and what a wrong kernel would add to it."""
    h, out = h0, []
    for t in range(X.shape[1]):
        h = torch.tanh(torch.einsum('fg,bgn->bfn', W, X[:, t]) + torch.einsum('fg,bgn->bfn', V, h))
        if leak == 'batch':                                     # a stray read of the next sequence's input, times zero
            h = h + 0.0 * X[:, t].roll(-1, 0).sum(1, keepdim=True)
        elif leak == 'future' and t + 1 < X.shape[1]:           # a stray read of the next step's input, times zero
            h = h + 0.0 * X[:, t + 1].sum(1, keepdim=True)
        out.append(h)
    H = torch.stack(out, 1)
    return {'H': torch.nan_to_num(H, nan=0.5) if leak == 'launder' else H}


def test_checker_accepts_a_clean_kernel():
    X, h0, W, V = _fake_problem()
    done = assert_contract(lambda x, h: _fake_kernel(x, h, W, V), X, h0, {'H': 'bt.n'}, 2, reversal=True)
    assert done == [('P1', 1), ('P2', 1), ('P3', 1), ('P4', 1), ('P2', 4), ('P1', 2)]
    assert _runs_for(260) == list(RUNS) and _runs_for(3) == [('P1', 1), ('P2', 1), ('P3', 1), ('P4', 1), ('P2', 2)]


@pytest.mark.parametrize('leak,line', [('batch', '(I) isolation'), ('future', '(C) causality'), ('launder', '(N) no laundering')])
def test_checker_rejects_a_kernel_that_breaks_one_line(leak, line):
    X, h0, W, V = _fake_problem()
    with pytest.raises(AssertionError) as e:
        assert_contract(lambda x, h: _fake_kernel(x, h, W, V, leak), X, h0, {'H': 'bt.n'}, 2)
    assert line in str(e.value) and "'H'" in str(e.value), str(e.value)


def test_checker_rejects_a_reversed_batch_that_differs_and_a_finite_gradient():
    X, h0, W, V = _fake_problem()

    def by_position(x, h):                                      # sequence 0 is computed differently: position-dependent, yet isolated
        H = _fake_kernel(x, h, W, V)['H'].clone()
        H[0] = H[0] * (1 + 2.0 ** -40)
        return {'H': H}
    with pytest.raises(AssertionError) as e:
        assert_contract(by_position, X, h0, {'H': 'bt.n'}, 2, reversal=True)
    assert '(R)' in str(e.value)

    def drops_the_item(x, h):                                   # a weight gradient that leaves the poisoned sequence out of its sum
        H = _fake_kernel(x, h, W, V)['H']
        keep = torch.isfinite(H).all(dim=(1, 2, 3))
        return {'H': H, 'grad:weight_A': torch.einsum('btfn,btgn->fg', H[keep], x[keep])}
    with pytest.raises(AssertionError) as e:
        assert_contract(drops_the_item, X, h0, {'H': 'bt.n'}, 2)
    assert '(N)' in str(e.value) and 'grad:weight_A' in str(e.value)


# ================================================================================================================== the rows
def _wanted(c):
    """The rows of the issue as a predicate over CASES (tests/test_poisoned_workspace.py)."""
    e = c.env
    nopack = e.get('GCRNN_NO_INLINE_PACK') == '1'
    selfstart = e.get('GCRNN_SEQ32_SELF_START')
    if c.path == 'fused' and c.graph == 'uniform' and c.shape in ('U400', 'U1000'):
        if 'GCRNN_SEQ32_STATE_SCRATCH' in e or c.hz or selfstart == '1':
            return False
        if c.sg is not None:                                    # node, time+node, edge: the wide passes and the 16-feature passes
            return not nopack and not c.last_only
        if c.kind == 'head':                                    # un-gated, time-gated, with and without self-start
            return True
        if c.last_only:
            return c.kernel in ('wide', 'step') and selfstart is None
        return c.kernel == 'wide' or not nopack                 # every kernel; the wide rows also without the inline pack and without self-start
    if c.path == 'fused' and c.shape in ('U204', 'G1', 'F20'):
        return True
    if c.path == 'fused' and c.graph in ('rank1', 'weighted'):
        return c.gating in ('none', 'time')
    if c.path == 'train':
        if nopack:
            return False
        return c.kind == 'train_head' or c.shape == 'U400' or c.gating in ('none', 'time')
    if c.kind == 'native' or c.path == 'stream':
        return True
    if c.path == 'x3':
        if c.hz:
            return False
        if c.graph == 'rank1':
            return c.id == 'x3-fwd-none-X400-rank1'
        if c.mode == 'train':
            return c.shape == 'X400'
        return c.shape == 'X400' or c.gating in ('none', 'time')
    if c.path == 'small' and c.graph == 'adj59':
        if c.kind in ('classify', 'regress') and c.gating != 'none':
            return False
        if c.prec == 'f64':                                     # one fp64 row of each family: its training row (with dX where there is one)
            return c.mode == 'train' and c.gating in ('none', 'edge') and (c.gating != 'edge' or c.dx)
        return True
    return False


def _rows():
    out = []
    for c in CASES:
        if not _wanted(c):
            continue
        r = copy.copy(c)
        r.env = dict(c.env)
        if c.path != 'stream':                                  # (streaming: the table's sizes)
            dims = dict(N=c.N, F=c.F, G=c.G, Kin=c.Kin, Kst=c.Kst, B=BATCH, T=c.T if c.path == 'small' else STEPS)
            r.__dict__.update(dims)                             # (what dims= of Case does)
            r.id = '%s-B%d' % (c.id, BATCH)
        out.append(r)
    return out


ROWS = _rows()


def test_row_table_covers_the_issue():
    """CPU: every line of the row list is present, ids are unique, and no row is smaller than it should be."""
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids)
    by = lambda **kw: [r for r in ROWS if all(getattr(r, k) == v for k, v in kw.items())]
    env = lambda rows, k, v: [r for r in rows if r.env.get(k) == v]
    for r in ROWS:
        N, F, G, K = (SHAPES[r.shape][:4] if r.shape in SHAPES else (r.N, r.F, r.G, r.K))
        assert (r.N, r.F, r.G, r.K) == (N, F, G, K), r.id
        assert (r.B, r.T) == ((3, 3) if r.path == 'stream' else (BATCH, 4 if r.path == 'small' else STEPS)), r.id
        assert r.route is not None, r.id
    for shape in ('U400', 'U1000'):
        fused = by(path='fused', shape=shape, graph='uniform')
        plain = [r for r in fused if r.kind == 'cell' and not r.last_only and r.sg is None and not env([r], 'GCRNN_NO_INLINE_PACK', '1')
                 and not env([r], 'GCRNN_SEQ32_SELF_START', '0')]
        assert sorted((r.kernel, r.gating) for r in plain) == sorted([(k, g) for k in ('wide', 'seq16', 'step') for g in ('none', 'time')] + [('hop', 'none')])
        assert sorted(r.gating for r in env(fused, 'GCRNN_NO_INLINE_PACK', '1')) == ['none', 'time'] and all(r.kernel == 'wide' for r in env(fused, 'GCRNN_NO_INLINE_PACK', '1'))
        assert [r.kernel for r in env(fused, 'GCRNN_SEQ32_SELF_START', '0') if r.kind == 'cell'] == ['wide']
        assert sorted((r.kernel, r.gating) for r in fused if r.last_only) == sorted((k, g) for k in ('wide', 'step') for g in ('none', 'time'))
        heads = [r for r in fused if r.kind == 'head']
        assert [r for r in heads if r.self_start] and env(heads, 'GCRNN_SEQ32_SELF_START', '0') and [r for r in heads if r.tg]
        for gating in ('node', 'time+node', 'edge'):
            rows = by(path='fused', shape=shape, graph='uniform', gating=gating)
            assert env(rows, 'GCRNN_SEQ32', '0') and env(rows, 'GCRNN_SEQ32_MIN_B', '1'), (shape, gating)
        for chain in ('wide', 'step'):
            for gating in ('none', 'time') + (('node', 'time+node', 'edge') if shape == 'U400' else ()):
                rows = by(path='train', shape=shape, kernel=chain, gating=gating, kind='cell')
                assert rows and all(r.dx == (r.sg is None) and r.dh0 == (r.sg is None) for r in rows), (shape, chain, gating)
    for gating in ('none', 'time'):
        assert by(kind='train_head', gating=gating) and by(kind='native', gating=gating)
        for graph in ('rank1', 'weighted'):
            assert by(path='fused', shape='U1000', graph=graph, gating=gating)
        assert by(path='x3', shape='X1000', gating=gating, mode='infer') and by(path='x3', shape='X400', gating=gating, mode='train')
    assert len(by(shape='U204')) == 4 and len(by(shape='G1')) == 5 and len(by(shape='F20')) == 4
    for gating in ('none', 'time', 'node', 'edge'):
        assert by(path='x3', shape='X400', gating=gating, mode='infer', graph='uniform')
    assert len(by(path='x3', graph='rank1')) == 1 and by(path='x3', graph='rank1')[0].mode == 'infer'
    assert len(by(path='stream')) == 3
    small = by(path='small', graph='adj59', prec='f32')
    for mode in ('infer', 'train'):
        assert sorted(r.gating for r in small if r.family == 'mfma' and r.kind == 'cell' and r.mode == mode) == ['node', 'none', 'time']
        assert sorted(r.gating for r in small if r.family == 'gather' and r.mode == mode) == ['none', 'time']
        for kind in ('classify', 'regress'):
            assert [r.gating for r in small if r.kind == kind and r.mode == mode] == ['none']
    assert sorted((r.mode, r.dx) for r in small if r.gating == 'edge') == [('infer', False), ('train', False), ('train', True)]
    f64 = by(path='small', prec='f64')
    assert sorted((r.family, r.kind, r.gating) for r in f64 if r.gating != 'edge') == [('gather', 'cell', 'none'), ('mfma', 'cell', 'none'), ('mfma', 'classify', 'none'), ('mfma', 'regress', 'none')]
    assert len([r for r in f64 if r.gating == 'edge']) == 1 and len(f64) == 5
    assert not [r for r in ROWS if r.hz]                        # (P3 runs on every row)


def _fresh(p, X, h0):
    """The one build with this run's inputs: gradients of the earlier runs dropped, the head's tensors cloned."""
    for cell in (p.cell, p.cell2):
        if cell is not None:
            for q in cell.parameters():
                q.grad = None
    head = None if p.head is None else [t.detach().clone() for t in p.head]
    return types.SimpleNamespace(cell=p.cell, cell2=p.cell2, X=X, h0=h0, dOut=p.dOut, head=head, S=p.S)


@pytest.mark.gpu
@pytest.mark.parametrize('row', ROWS, ids=[r.id for r in ROWS])
def test_a_non_finite_input_stays_in_its_sequence_and_step(row, monkeypatch):
    c = row
    _set_env(monkeypatch, c.env)
    p = _build(c)                                               # once: cell, graph operator (its plans are cached on it), inputs

    def run(X, h0):
        return _run_kernels(c, _fresh(p, X, h0))                # (calls the row's route first: the kernel of the id is the one that ran)
    done = assert_contract(run, p.X, p.h0, layouts_of(c), node_with_a_neighbour(_gso(c.graph, c.N)), skip_p3=c.hz, reversal=c.mode == 'infer')
    assert len(done) == (6 if c.B > 257 else 5), done


# ================================================================================================================== stand-alone ops
#   maker -> (operand, index of the poisoned element, {output: the axes that name the item -- the same axes in the output as in the operand},
#   {output: index that must be non-finite}); an output not listed sums over the items (dw, db) and is not compared.
def _op_spec(make, args):
    if make is _op_graph_filter_layer:
        return 'x', (2, 0, 7), {'y': (0,), 'dx': (0,)}, {'y': (2, slice(None), 7)}
    if make is _op_node_linear:
        return 'h', (3, 0, 5), {'y': (0,), 'dh': (0,)}, {'y': (3, slice(None), 5)}
    if make is _op_rnn_sequence:                                # per sequence, and causal in t: H[b0, :t0] of the clean run
        return 'x', (1, T0, 0), {'H': (0,), 'dx': (0,), 'dh0': (0,)}, {'H': (1, slice(T0, None))}
    if make is _op_edge_attention:                              # [T][N][B][F]: the item is (t, b). Node 3's one edge in S + I is its own loop, with
        #                                                         alpha = 1: y[3] = Wx[3] (node 5 would not do: (S + I)[5][5] = 0 there, no edge)
        return 'Wx', (1, 3, 1, 0), {'y': (0, 2), 'dWx': (0, 2), 'ds1': (0, 2), 'ds2': (0, 2)}, {'y': (1, 3, 1, 0)}
    if make is _op_lsigf_two_edge_features:
        return 'x', (1, 0, 7), {'y': (0,), 'dx': (0,)}, {'y': (1, slice(None), 7)}
    if make is _op_cross_entropy:
        return 'z', (1, 0), {'dz': (0,)}, {'loss': ()}
    if make is _op_l1_loss:                                     # element by element
        return 'x', (1, 0, 0, 0), {'dx': (0, 1, 2, 3), 'dy': (0, 1, 2, 3)}, {'loss': ()}
    if make is _op_batch_time_mse:                              # mixes every row by definition: non-finite in, non-finite out
        return 'x', (1, 0), {}, {'metric': ()}
    raise KeyError(make)


def check_op(clean, got, index, items, nonfinite):
    for name, axes in items.items():
        a, c = got[name], clean[name]
        assert a.shape == c.shape and a.dtype == c.dtype, name
        other = torch.zeros(a.shape, dtype=torch.bool, device=a.device)
        for ax in axes:                                         # (an element of another item differs from the poisoned one in some item coordinate)
            coord = torch.arange(a.shape[ax], device=a.device).view([-1 if d == ax else 1 for d in range(a.dim())])
            other |= coord != index[ax]
        if not torch.equal(a[other], c[other]):
            raise AssertionError('(I) isolation: output %r differs from the clean run outside the poisoned item %r, first at %s' % (
                name, tuple(index[ax] for ax in axes), _first(other & ((a != c) | a.isnan()))))
    for name, at in nonfinite.items():
        part = got[name][at] if at != () else got[name]
        assert not bool(torch.isfinite(part).any()), '(N) no laundering: output %r at %r holds finite values' % (name, at)


def test_op_checker_bites():
    clean = {'y': torch.arange(12.0).reshape(3, 4), 'loss': torch.tensor(1.0)}
    bad = {'y': clean['y'].clone(), 'loss': torch.tensor(NAN)}
    bad['y'][1] = NAN
    check_op(clean, bad, (1, 0), {'y': (0,)}, {'y': (1,), 'loss': ()})
    leak = {k: v.clone() for k, v in bad.items()}
    leak['y'][2, 3] += 1
    with pytest.raises(AssertionError) as e:
        check_op(clean, leak, (1, 0), {'y': (0,)}, {'y': (1,), 'loss': ()})
    assert '(I)' in str(e.value) and '(2, 3)' in str(e.value)
    with pytest.raises(AssertionError) as e:
        check_op(clean, dict(bad, loss=torch.tensor(2.0)), (1, 0), {'y': (0,)}, {'y': (1,), 'loss': ()})
    assert '(N)' in str(e.value)
    assert {m for _, m, _ in OPS} == {_op_graph_filter_layer, _op_node_linear, _op_rnn_sequence, _op_edge_attention, _op_lsigf_two_edge_features,
                                     _op_cross_entropy, _op_l1_loss, _op_batch_time_mse}
    for _, m, a in OPS:
        _op_spec(m, a)


@pytest.mark.gpu
@pytest.mark.parametrize('make,args', [(m, a) for _, m, a in OPS], ids=[i for i, _, _ in OPS])
def test_a_non_finite_element_stays_in_its_row_of_the_op(make, args, monkeypatch):
    _set_env(monkeypatch, {})
    run, _ = make(*args)
    operand, index, items, nonfinite = _op_spec(make, args)
    clean = run()
    for name, t in clean.items():
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), name
    hit = []

    def edit(operands):
        operands[operand][index] = NAN
        hit.append(operand)
    got = run(edit=edit)
    assert hit == [operand]
    check_op(clean, got, index, items, nonfinite)
    if make is _op_rnn_sequence:
        assert torch.equal(got['H'][index[0], :T0], clean['H'][index[0], :T0]), '(C) causality: H[b0, :t0] differs from the clean run'


# ================================================================================================================== ReLU keeps a NaN
@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_relu_keeps_a_nan(prec, monkeypatch):
    """torch.relu(NaN) is NaN; `v > 0 ? v : 0` and fmaxf(v, 0) are 0. The two stand-alone ops with a ReLU of their own (the GNN heads'
    graph-filter layer, the RNN baseline) against plain torch in fp64 on the poisoned operand: where the reference is non-finite the
    kernel is, and every other item is the clean run's bit for bit. (The edge gate's ReLU is on the cell rows above.)"""
    from conftest import GOLDEN
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator
    from test_poisoned_workspace import DEV
    from test_rnn_baseline import _case, torch_rnn
    import os
    _set_env(monkeypatch, {})
    dt = {'f32': torch.float32, 'f64': torch.float64}[prec]
    with torch.no_grad():
        # ---- graph_filter_layer, N = 59, hops first and taps first
        S = np.load(os.path.join(GOLDEN, 'adj59.npy'))
        S = (S / np.max(np.abs(np.linalg.eigvals(S)))).reshape(1, 59, 59)
        graph = GraphOperator(S, device=DEV)
        Sd = torch.tensor(S[0], dtype=torch.float64, device=DEV)
        m0 = node_with_a_neighbour(S)
        for Fin, Fout, K in ((20, 1, 4), (20, 21, 4)):
            assert ops.graph_filter_layer_supported(dt, dt, graph, Fin, Fout, K)
            g = torch.Generator().manual_seed(Fin + Fout)
            x = torch.randn(5, Fin, 59, generator=g, dtype=torch.float64).to(dt).to(DEV)
            w = (torch.randn(Fout, 1, K, Fin, generator=g, dtype=torch.float64) / np.sqrt(Fin * K)).to(dt).to(DEV)
            b = torch.randn(Fout, 1, generator=g, dtype=torch.float64).to(dt).to(DEV)
            clean = ops.graph_filter_layer(x, w, b, graph, 'relu')
            xp = x.clone()
            xp[2, 0, m0] = NAN
            got = ops.graph_filter_layer(xp, w, b, graph, 'relu')
            # the reference on the SUPPORT of S (a dense x @ S spreads 0 * NaN to every node; the kernels gather along edges, as P4's note says):
            # a node is non-finite where a walk of < K edges from m0 reaches it, node m0 itself through tap 0
            reach = torch.zeros(59, dtype=torch.float64, device=DEV)
            reach[m0] = 1.0
            hit = reach.clone()
            for k in range(1, K):
                reach = reach @ (Sd != 0).double()
                hit = hit + reach
            assert bool(hit[m0] > 0) and int((hit > 0).sum()) > 1 and bool(torch.isfinite(clean).all())
            assert not bool(torch.isfinite(got[2][:, hit > 0]).any()), '(N) graph_filter_layer: finite where the NaN reaches'
            assert torch.equal(got[:2], clean[:2]) and torch.equal(got[3:], clean[3:]), '(I) graph_filter_layer'
    # ---- rnn_sequence with ReLU: per sequence, causal in t
    B, T, D, Fh = 67, 3, 22, 9
    assert ops.rnn_supported(dt, B, T, D, Fh)
    ts, ks, _ = _case(B, T, D, Fh, 'relu', True, dt, seed=5)
    with torch.no_grad():
        clean = ops.rnn_sequence(*ks, 'relu')
        ks[0][1, T0, 0] = NAN
        ts[0][1, T0, 0] = NAN
        got = ops.rnn_sequence(*ks, 'relu')
        ref = torch_rnn(*ts, 'relu')
    assert bool(ref[1, T0:].isnan().all()) and bool(torch.isfinite(clean).all())
    assert not bool((torch.isfinite(got) & ~torch.isfinite(ref)).any()), '(N) rnn_sequence: finite where the reference is not'
    assert torch.equal(got[:1], clean[:1]) and torch.equal(got[2:], clean[2:]), '(I) rnn_sequence'
    assert torch.equal(got[1, :T0], clean[1, :T0]), '(C) rnn_sequence'
