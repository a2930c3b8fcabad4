"""The time-gated kernels at zero, underflowed and saturated gates.

Every time-gated kernel on the hot path builds gi (A(S)x + b) + gf (B(S)h + b) on ONE accumulator chain (h-chain, scale by gf / gi, x-chain,
scale by gi), guarded by wave-uniform comparisons against 1e-30 (csrc/gcrnn_fused_seq32.h, gcrnn_fused_step.h, gcrnn_fused_seq.h). The rest
of the suite draws its gates from a freshly initialised gate sub-network or from uniform(0.2, 0.9): no guarded branch is ever taken. Here
the gates are PRESCRIBED (ops.fused_cell_forward(gate_values=), ops.fused_cell_train_with_gates), one regime per sequence of one launch,
every sequence on the same X and h0 (GATE_TABLE below), against a dense fp64 recurrence with explicit gates that is tied on the CPU to
oracle/gcrnn_oracle.py (states) and oracle/torch_reference.py (gradients under autograd).

Which row of the table reaches which guarded branch, on each of the three bf16 forward kernels (wide, 16-feature sequence-resident, step),
and the check that fails under the neighbouring wrong branch:
  xpart false (gi <= 1e-30: the x-chain is skipped)        rows 1, 3, 4, 12, 13   H bit-identical under another X (rows 1, 3); row 1 is 0.69+ from row 10
  hpart false (gf <= 1e-30 on the hop sums) / gratio = 0    rows 2, 3, 11 (t = 2)  H bit-identical under another h0; row 2 is 0.22+ from row 10
  ratio gf / gi = 1e29 (gi just above the guard)           row 5                  rows 5 and 6 are 0.98+ apart (the two chains swapped)
  1 / gf = 1e29 on the hop sums                            row 6                  the same pair; H finite
  S / gf huge at ratio 1                                   row 7                  |H - reference| (H is ~1e-20)
  the comparison itself, a denormal gate                   rows 12, 13            finite and within the bound (either side of the guard is right)
Before any launch the CPU proves from the reference alone that those pairs are at least MARGIN = 20 bounds apart.

Bounds: those the same kernels carry in tests/test_directed_uniform.py and tests/test_fused.py, per ROW of the table (a row is a sequence of
its own): |H - reference| <= 6e-3 max, 1e-3 mean (_h_bounds, time-gated); the head ||w||_1 x 6e-3; gradients 5e-2 max / 1e-2 mean of the
gradient's max (_grad_scale_and_bounds), d gi / d gf / d X / d h0 of a regime on THAT regime's reference magnitude.

C runs the same cells with the gates saturated through their own sub-networks (read-out biases -120 .. +120), D saturates four state features
through the cell's bias (+-100), each on every path that carries the cell: bf16 fused (gate pair and per-gate pre-passes; wide, 16-feature and
step kernels; both BPTT chains), fp32-accurate x3, one-launch small-graph kernels, bf16 streaming Horner.

One floor is coarser than the forward's: the bf16 weight-gradient kernel leaves out items whose gate is <= 1e-12. With every
gate of a batch in (1e-30, 1e-12] its weight_A / weight_B gradient is 0 where the reference's is ~1e-27; C holds it to that floor
(WGRAD_GATE_FLOOR x the open-gate gradient), every other gradient relatively. The x3 and small-graph paths meet the relative bound there.

Measured on an MI355X (GCRNN_TOL_REPORT; worst case of each group next to its bound):
  A forward |H - reference|, worst ROW: wide 2.7e-3 max, 5.1e-4 mean; 16-feature and step 2.5e-3, 4.7e-4 (6e-3 / 1e-3); rows 3, 7, 13: 0, 1.6e-20,
    1.6e-30; head 3.5e-3 (||w||_1 x 6e-3 = 1.9e-2). Every exact invariant holds on all three kernels and the head form.
  B BPTT, of each gradient's max: weight_A / weight_B / bias <= 2.8e-3 (5e-2), mean <= 9.1e-4 (1e-2); worst REGIME on its own magnitude: d X 7.5e-3,
    d h0 4.2e-3, d gi 7.1e-3, d gf 7.8e-3 (5e-2), wide and step chain alike; the exact zeros hold; head chain == chain, bit for bit.
  C sub-network gates: bf16 H 2.6e-3 max, 4.2e-4 mean (6e-3 / 1e-3), live gradients <= 1.3e-2 (5e-2 class bounds); x3 H 2.8e-7 (1e-5), gradients
    2.7e-6 (2e-5); small graph fp64 H 8.4e-15 (1e-11), gradients 7.7e-15 (1e-9); fp32 H 3.4e-6 (1e-5), gradients 2.6e-6 (5e-4); every dead
    gate-parameter gradient is finite and <= 1e-20.
  D saturated states: +-1 exactly on every path; other features wide 3.1e-3 / 5.4e-4, 16-feature and step 2.5e-3 / 4.9e-4 (5e-3 .. 6e-3 / 1e-3), x3 3.7e-7
    (1e-5), small graph 1.7e-6 (1e-5), streaming Horner 3.4e-3 / 7.2e-4 (5e-2 / 4e-3); gradients bf16 5.2e-3 (5e-2), x3 6.2e-7 (2e-5), small graph
    9.4e-7 (5e-4); dpre exactly 0 on the saturated features. Nothing here contradicts the "abs error < 3e-7" beside fast_tanh / act_tanh.
No kernel had to change and no bound is wider than the existing test of the same kernel."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from oracle import torch_reference as tref
from test_directed_uniform import FORWARD_ENV, MARGIN, _h_bounds, _head_weights, _setenv, bf16_round, f32_round
from test_fp64_envelopes import _CountingLib
from test_fused import _grad_scale_and_bounds, _tol_report
from test_wide import _uniform_cell

SMALL = (400, 32, 32, 3)          # (N, F, G, K): one 32-feature chunk per step
LARGE = (1000, 64, 64, 5)         # two chunks per step
T = 4
SEED = 91
H0_STD = 0.3

# one regime per sequence: (gi, gf) held over the T steps; row 11 shuts the forget gate at t = 2 only
GATE_TABLE = [(1.0, 1.0), (0.0, 0.7), (0.6, 0.0), (0.0, 0.0), (1e-35, 0.7), (1e-29, 1.0), (1.0, 1e-29), (1e-20, 1e-20), (1e-8, 1.0),
              (1.0, 1e-8), (0.6, 0.6), (0.6, 0.6), (5e-39, 0.5), (1e-30, 1e-30)]
B = len(GATE_TABLE)
RESET_ROW, RESET_STEP = 11, 2
X_DROPPED = (1, 3)                # gi = 0: no bit of H may depend on X
H_DROPPED = (2, 3)                # gf = 0: ... on h0
UNTOUCHED = (0, 10)
GRAD_MAX, GRAD_MEAN = 5e-2, 1e-2  # the bf16 class gates of tests/test_fused.py / tests/test_directed_uniform.py
TINY = 1e-36                      # absolute floor of a per-regime gradient comparison: below every normal-float regime of the table (a
                                  # denormal gate times an O(1) sum may flush)


def gate_table():
    """(gi, gf) [T][B] fp32: what the kernels are handed, and what the reference reads (as fp64)."""
    gi = np.tile(np.array([r[0] for r in GATE_TABLE], dtype=np.float32), (T, 1))
    gf = np.tile(np.array([r[1] for r in GATE_TABLE], dtype=np.float32), (T, 1))
    gf[RESET_STEP, RESET_ROW] = 0.0
    return gi, gf


# ------------------------------------------------------------------------------------------------------------ references
def gated_cell(params, S, X, h0, gi, gf):
    """h_t = tanh(gi[t][b] (A(S) x_t + b) + gf[t][b] (B(S) h_{t-1} + b)), dense, in the dtype of its inputs (fp64): B x T x F x N."""
    Bn = X.shape[0]
    h, H = h0, []
    for t in range(X.shape[1]):
        ya = orc.lsigf(params['weight_A'], S, X[:, t], params['bias'])
        yb = orc.lsigf(params['weight_B'], S, h, params['bias'])
        h = np.tanh(np.asarray(gi[t]).reshape(Bn, 1, 1) * ya + np.asarray(gf[t]).reshape(Bn, 1, 1) * yb)
        H.append(h)
    return np.stack(H, axis=1)


def gated_cell_torch(P, S, X, h0, gi, gf):
    """The same recurrence on torch tensors (autograd gives the gradients w.r.t. everything, the gates included)."""
    Bn = X.shape[0]
    h, H = h0, []
    for t in range(X.shape[1]):
        ya = tref.lsigf(P['weight_A'], S, X[:, t], P['bias'])
        yb = tref.lsigf(P['weight_B'], S, h, P['bias'])
        h = torch.tanh(gi[t].reshape(Bn, 1, 1) * ya + gf[t].reshape(Bn, 1, 1) * yb)
        H.append(h)
    return torch.stack(H, dim=1)


def oracle_time_gates(params, S, X, h0):
    """The oracle's own time gates (gi, gf) [T][B]: sigmoid(Linear(tanh-cell(x_t, h0))) of the two gate sub-networks."""
    Bn, Tn = X.shape[0], X.shape[1]
    out = []
    for name in ('in', 'forget'):
        sub = orc._sub(params, 'GFL_%s.' % name)
        g = [orc.sigmoid(orc._plain_step(sub, S, X[:, t], h0, np.tanh).reshape(Bn, -1) @ params['MLP_%s.0.weight' % name].T
                         + params['MLP_%s.0.bias' % name]).reshape(Bn) for t in range(Tn)]
        out.append(np.stack(g, axis=0))
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """One problem per shape, computed once and never written to: the un-gated cell of test_wide._uniform_cell (bf16 parameters on a
    uniform-weight graph), ONE bf16-representable (X, h0) shared by all B sequences, the gate table, and the fp64 reference states."""
    N, F, G, K = shape
    cell, rng, S = _uniform_cell(N, G, F, K, SEED + N)
    state = {k: v.detach().float().clone() for k, v in cell.state_dict().items()}
    params = {k: v.double().numpy() for k, v in state.items()}
    x1 = bf16_round(rng.standard_normal((1, T, G, N)))
    h1 = bf16_round(H0_STD * rng.standard_normal((1, F, N)))
    X, h0 = np.repeat(x1, B, axis=0), np.repeat(h1, B, axis=0)
    X2, h02 = X.copy(), h0.copy()                               # the second launch: one operand changed per invariant
    for b in X_DROPPED:
        X2[b] = bf16_round(2.0 * rng.standard_normal((T, G, N)))
    for b in H_DROPPED + (RESET_ROW,):
        h02[b] = bf16_round(H0_STD * rng.standard_normal((F, N)))
    R = bf16_round(rng.standard_normal((B, T, F, N)))
    gi, gf = gate_table()
    S32 = f32_round(S)
    H = gated_cell(params, S32, X, h0, gi.astype(np.float64), gf.astype(np.float64))
    for a in (X, h0, X2, h02, R, H, gi, gf):
        a.setflags(write=False)
    return types.SimpleNamespace(shape=shape, N=N, F=F, G=G, K=K, S=S, S32=S32, state=state, params=params, X=X, h0=h0, X2=X2, h02=h02,
                                 R=R, gi=gi, gf=gf, H=H, tg=True, sg=None)


@functools.lru_cache(maxsize=None)
def _case_grads(shape):
    """Reference gradients of loss = sum(H * R) under torch autograd in fp64: parameters, X, h0 and BOTH gates."""
    c = _case(shape)
    t64 = lambda a, g=True: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=g)
    P = {k: t64(v) for k, v in c.params.items()}
    X, h0, gi, gf = t64(c.X), t64(c.h0), t64(c.gi), t64(c.gf)
    H = gated_cell_torch(P, t64(c.S32, False), X, h0, gi, gf)
    (H * t64(c.R, False)).sum().backward()
    g = {k: v.grad.numpy() for k, v in P.items()}
    g.update(dX=X.grad.numpy(), dh0=h0.grad.numpy(), dgi=gi.grad.numpy(), dgf=gf.grad.numpy())
    return g


def _separation(c, a, b, steps=slice(None)):
    return float(np.abs(c.H[a, steps] - c.H[b, steps]).max())


def _assert_rows_discriminate(c, tol):
    """CPU, from the reference alone: a wrong branch moves H by at least MARGIN bounds."""
    V = c.H
    for a, b, steps, what in ((1, 10, slice(None), 'the x-chain kept where it must be dropped'), (2, 10, slice(None), 'the h-chain kept or dropped'),
                              (5, 6, slice(None), 'the two chains swapped'), (RESET_ROW, 10, slice(RESET_STEP, None), 'no reset in mid-sequence')):
        d = float(np.abs(V[a, steps] - V[b, steps]).max())
        assert d >= MARGIN * tol, '%s: rows %d and %d are %.3g apart only, %.1f x the bound %.3g' % (what, a, b, d, d / tol, tol)
    assert np.array_equal(V[RESET_ROW, :RESET_STEP], V[10, :RESET_STEP])


# ------------------------------------------------------------------------------------------------------------ CPU
def _small_problem(tg):
    import gated_gcrnns_amd.Utils.graphML as gml
    N, F, G, K, Bn, Tn = 30, 6, 5, 3, 3, 4
    rng = np.random.default_rng(5)
    W = (rng.random((N, N)) < 0.2) * rng.uniform(0.2, 1.0, (N, N))
    S = (W / np.linalg.norm(W, 2)).reshape(1, N, N)
    torch.manual_seed(5)
    cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, tg, None, 1, True).double()
    cell.addGSO(torch.tensor(S))
    params = {k: v.detach().numpy().copy() for k, v in cell.state_dict().items()}
    return params, S, rng.standard_normal((Bn, Tn, G, N)), 0.4 * rng.standard_normal((Bn, F, N))


def test_explicit_gate_recurrence_is_the_oracles_cell():
    """CPU: the dense recurrence with explicit gates equals oracle.ggcrnn_cell -- un-gated at gi = gf = 1, and time-gated when fed the
    oracle's own gates -- to 1e-12; the gates it is fed there are not trivial."""
    params, S, X, h0 = _small_problem(True)
    one = np.ones((X.shape[1], X.shape[0]))
    assert np.abs(gated_cell(params, S, X, h0, one, one) - orc.ggcrnn_cell(params, S, X, h0)).max() <= 1e-12
    gi, gf = oracle_time_gates(params, S, X, h0)
    assert gi.std() > 1e-3 and gf.std() > 1e-3 and np.abs(gi - gf).max() > 1e-3
    Hg = orc.ggcrnn_cell(params, S, X, h0, time_gating=True)
    assert np.abs(gated_cell(params, S, X, h0, gi, gf) - Hg).max() <= 1e-12
    assert np.abs(Hg - orc.ggcrnn_cell(params, S, X, h0)).max() > 1e-2


def test_explicit_gate_recurrence_in_torch_is_the_torch_references_cell():
    """CPU: the same for the torch restatement and oracle/torch_reference.ggcrnn_cell, states AND gradients (to 1e-12 of each gradient's
    max); with the gates detached the time-gated parameter gradients of the main cell still agree (they do not pass through the gates)."""
    params, S, X, h0 = _small_problem(True)
    rng = np.random.default_rng(6)
    R = torch.tensor(rng.standard_normal((X.shape[0], X.shape[1], h0.shape[1], h0.shape[2])))
    t64 = lambda a, g=False: torch.tensor(a, dtype=torch.float64, requires_grad=g)
    gates = [t64(g) for g in oracle_time_gates(params, S, X, h0)]
    one = torch.ones((X.shape[1], X.shape[0]), dtype=torch.float64)
    for tg, (gi, gf) in ((False, (one, one)), (True, gates)):
        got, want = [], []
        for mine, out in ((True, got), (False, want)):
            P = {k: t64(v, True) for k, v in params.items()}
            Xt = t64(X, True)
            H = gated_cell_torch(P, t64(S), Xt, t64(h0), gi, gf) if mine else tref.ggcrnn_cell(P, t64(S), Xt, t64(h0), tg)
            (H * R).sum().backward()
            out.extend([H.detach(), P['weight_A'].grad, P['weight_B'].grad, P['bias'].grad] + ([] if tg else [Xt.grad]))
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # the numpy and the torch recurrence are one function
    assert np.abs(gated_cell(params, S, X, h0, gates[0].numpy(), gates[1].numpy())
                  - gated_cell_torch({k: t64(v) for k, v in params.items()}, t64(S), t64(X), t64(h0), *gates).numpy()).max() <= 1e-12


def test_gate_table_holds_the_values_the_guards_decide_on():
    """CPU: the table as fp32 -- what is below, at and above the kernels' 1e-30f, which entry is a denormal, where the reset sits."""
    gi, gf = gate_table()
    guard, tiny = np.float32(1e-30), np.finfo(np.float32).tiny
    assert gi.shape == gf.shape == (T, B) and B == 14 and gi.dtype == np.float32
    assert np.all(gi[:, [1, 3]] == 0) and np.all(gf[:, [2, 3]] == 0)
    assert tiny < gi[0, 4] < guard and 0 < gi[0, 12] < tiny                      # a normal float below the guard; a denormal
    assert gi[0, 5] > guard and gf[0, 6] > guard and gi[0, 5] < 1.01e-29         # just above it
    assert gi[0, 13] == guard and gf[0, 13] == guard                             # the comparison itself
    assert np.isfinite(np.float32(1.0) / gf[0, 6]) and np.isfinite(gf[0, 5] / gi[0, 5])      # 1e29: no overflow in the scales themselves
    assert np.array_equal(gi[:, RESET_ROW], gi[:, 10]) and gf[RESET_STEP, RESET_ROW] == 0
    assert np.array_equal(np.delete(gf[:, RESET_ROW], RESET_STEP), np.delete(gf[:, 10], RESET_STEP))
    assert all(np.all(g[0] == g[t]) for g in (gi,) for t in range(T))


@pytest.mark.parametrize('shape', [SMALL, LARGE])
def test_gate_regimes_discriminate_on_the_reference_alone(shape):
    """CPU, no launch: a kernel that takes the neighbouring wrong branch moves H by at least 20 bounds -- the pairs the
    GPU cases rely on; the zero-gate rows do not see the operand their gate shuts; row 3 is exactly 0; every sequence has the same data."""
    c = _case(shape)
    assert all(np.array_equal(c.X[b], c.X[0]) and np.array_equal(c.h0[b], c.h0[0]) for b in range(B)) and np.abs(c.h0).max() > 0
    assert np.array_equal(bf16_round(c.X), c.X) and np.array_equal(bf16_round(c.h0), c.h0)
    _assert_rows_discriminate(c, _h_bounds(c)[0])
    assert np.abs(c.H[3]).max() == 0.0 and np.abs(c.H[12]).max() > 0.1 and np.abs(c.H[13]).max() <= 1e-28
    H2 = gated_cell(c.params, c.S32, c.X2, c.h02, c.gi.astype(np.float64), c.gf.astype(np.float64))
    for b in X_DROPPED + H_DROPPED + UNTOUCHED:
        assert np.array_equal(H2[b], c.H[b]), b
    assert np.array_equal(H2[RESET_ROW, RESET_STEP:], c.H[RESET_ROW, RESET_STEP:])
    assert np.abs(H2[RESET_ROW, :RESET_STEP] - c.H[RESET_ROW, :RESET_STEP]).max() >= MARGIN * _h_bounds(c)[0]
    # (the changed operands do change something where the gate is open: row 10 fed row 1's other X would move)
    assert np.abs(c.X2[1] - c.X[1]).max() > 1 and np.abs(c.h02[2] - c.h0[2]).max() > 0.1


@pytest.mark.parametrize('shape', [SMALL, LARGE])
def test_zero_gates_still_have_derivatives_in_the_reference(shape):
    """CPU: what section B rests on -- the derivative with respect to a gate that is 0 is not 0, d X vanishes where gi = 0 and d h0 where
    gf = 0, and the reset row's d h0 does not."""
    c, g = _case(shape), _case_grads(shape)
    for b in (1, 3, 4):
        assert np.abs(g['dgi'][:, b]).max() > 1.0, b
    for b in (2, 3):
        assert np.abs(g['dgf'][:, b]).max() > 1.0, b
    assert all(np.abs(g['dX'][b]).max() == 0 for b in X_DROPPED) and all(np.abs(g['dh0'][b]).max() == 0 for b in H_DROPPED)
    assert np.abs(g['dh0'][RESET_ROW]).max() > 1e-3 and abs(g['dgf'][RESET_STEP, RESET_ROW]) > 1.0


# ------------------------------------------------------------------------------------------------------------ A. forward, prescribed gates
def _device_case(c, dtype):
    """The case's cell on the device (parameters in `dtype`) and its operands as bf16 tensors."""
    cell, _, _ = _uniform_cell(c.N, c.G, c.F, c.K, SEED + c.N)
    cell.load_state_dict(c.state)
    dev = torch.device('cuda:0')
    cell = cell.float().to(dev).to(dtype)
    bf = lambda a: torch.tensor(a, dtype=torch.bfloat16, device=dev)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    return cell, bf(c.X), bf(c.h0), bf(c.X2), bf(c.h02), f32(c.gi), f32(c.gf)


def _spy(monkeypatch):
    from gated_gcrnns_amd import ops
    s = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, 'lib', s)
    return s


WIDE_ENTRIES = ('gcrnn_fused_forward_wide_bf16', 'gcrnn_fused_forward_wide_scratch_bf16')
STEP_ENTRY = 'gcrnn_fused_forward_bf16'


def _rows_report(tag, c, err, mx, mn):
    per_max, per_mean = err.reshape(B, -1).max(axis=1), err.reshape(B, -1).mean(axis=1)
    line = 'gate extremes %s N=%d: |H - reference| worst row %d max %.3e, worst row %d mean %.3e (bounds %.1e / %.1e); per row max %s' % (
        tag, c.N, int(per_max.argmax()), per_max.max(), int(per_mean.argmax()), per_mean.max(), mx, mn, ' '.join('%.1e' % v for v in per_max))
    print(line)
    _tol_report(line)
    return per_max, per_mean


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('kernel', ['wide', 'seq16', 'step'])
def test_forward_with_prescribed_gates_matches_reference(kernel, shape, monkeypatch):
    """ops.fused_cell_forward(gate_values=(gi, gf)) on the gate table, on each bf16 forward kernel: every element finite, every ROW within
    the time-gated bound of the fp64 recurrence, and -- exactly -- no bit of H depends on an operand whose gate is 0 (a second launch with
    that operand replaced), while the rows that were not touched repeat their bits and the reset row's first steps do move."""
    from gated_gcrnns_amd import ops
    c = _case(shape)
    mx, mn = _h_bounds(c)
    assert (mx, mn) == (6.0e-3, 1.0e-3)
    _assert_rows_discriminate(c, mx)
    _setenv(monkeypatch, FORWARD_ENV[kernel])
    cell, Xd, hd, X2d, h2d, gi, gf = _device_case(c, torch.bfloat16)
    assert (ops.fused_wide_plan(cell.graph, B, T, c.N, c.F, c.G, c.K, False, rank1=True, gated=True) is not None) == (kernel == 'wide')
    spy = _spy(monkeypatch)
    with torch.no_grad():
        H = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, gate_values=(gi, gf))
        ran = dict(spy.calls)
        H2 = ops.fused_cell_forward(X2d, h2d, cell.weight_A, cell.weight_B, cell.bias, cell.graph, gate_values=(gi, gf))
    if kernel == 'wide':                                         # the intended kernel ran, and it alone
        assert sum(ran.get(n, 0) for n in WIDE_ENTRIES) == 1 and ran.get(STEP_ENTRY, 0) == 0, ran
    else:
        assert ran.get(STEP_ENTRY, 0) == 1 and sum(ran.get(n, 0) for n in WIDE_ENTRIES) == 0, ran
    assert H.dtype == torch.bfloat16 and tuple(H.shape) == (B, T, c.F, c.N)
    assert bool(torch.isfinite(H.float()).all()) and bool(torch.isfinite(H2.float()).all())
    err = np.abs(H.double().cpu().numpy() - c.H)
    per_max, per_mean = _rows_report(kernel, c, err, mx, mn)
    assert np.all(per_max <= mx) and np.all(per_mean <= mn), (per_max.tolist(), per_mean.tolist())
    for b in X_DROPPED + H_DROPPED + UNTOUCHED:
        assert torch.equal(H[b], H2[b]), 'row %d: H depends on an operand under a zero gate (or does not repeat)' % b
    assert torch.equal(H[RESET_ROW, RESET_STEP:], H2[RESET_ROW, RESET_STEP:])
    assert not torch.equal(H[RESET_ROW, 0], H2[RESET_ROW, 0]) and not torch.equal(H[RESET_ROW, 1], H2[RESET_ROW, 1])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SMALL, LARGE])
def test_wide_head_with_prescribed_gates_matches_reference(shape, monkeypatch):
    """The same table through ops.fused_cell_forward_wide_head (cell + Linear(F -> 1) as one launch): y against w . H_reference + b at
    ||w||_1 x the bound on H, row by row, with the head weights of test_directed_uniform_wide_head_matches_oracle."""
    from gated_gcrnns_amd import ops
    c = _case(shape)
    w = _head_weights(c.F)
    hb = float(np.float32(0.37))
    tol = float(np.abs(w).sum()) * _h_bounds(c)[0]
    yref = np.einsum('f,btfn->btn', w, c.H) + hb
    _setenv(monkeypatch, FORWARD_ENV['wide'])
    cell, Xd, hd, X2d, h2d, gi, gf = _device_case(c, torch.bfloat16)
    dev = Xd.device
    assert ops.fused_wide_head_supported(cell.graph, B, T, c.N, c.F, c.G, c.K, True)
    head = (torch.tensor(w, dtype=torch.float32, device=dev).view(1, c.F), torch.tensor([hb], dtype=torch.float32, device=dev))
    with torch.no_grad():
        y = ops.fused_cell_forward_wide_head(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head, gate_values=(gi, gf))
        y2 = ops.fused_cell_forward_wide_head(X2d, h2d, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head, gate_values=(gi, gf))
    assert tuple(y.shape) == (B, T, 1, c.N) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    e = np.abs(y[:, :, 0].double().cpu().numpy() - yref).reshape(B, -1).max(axis=1)
    line = 'gate extremes wide head N=%d: |y - head(H_reference)| worst row %d %.3e (bound %.3e)' % (c.N, int(e.argmax()), e.max(), tol)
    print(line); _tol_report(line)
    assert np.all(e <= tol), e.tolist()
    for b in X_DROPPED + H_DROPPED + UNTOUCHED:
        assert torch.equal(y[b], y2[b]), b
    assert torch.equal(y[RESET_ROW, RESET_STEP:], y2[RESET_ROW, RESET_STEP:]) and not torch.equal(y[RESET_ROW, :RESET_STEP], y2[RESET_ROW, :RESET_STEP])


# ------------------------------------------------------------------------------------------------------------ B. BPTT, prescribed gates
CHAIN_ENV = {'wide': {'GCRNN_SEQ32_MIN_B': '1'}, 'step': {'GCRNN_SEQ32_MIN_B': '1', 'GCRNN_NO_WIDE_CHAIN': '1'}}
WIDE_CHAIN, STEP_CHAIN = 'gcrnn_fused_backward_data_wide_bf16', 'gcrnn_fused_backward_data_bf16'


def _per_regime(name, got, ref, axis_b, missed, tag):
    """One gradient regime by regime, each on ITS OWN reference magnitude."""
    worst = 0.0
    for b in range(B):
        gb, rb = np.take(got, b, axis=axis_b), np.take(ref, b, axis=axis_b)
        assert np.all(np.isfinite(gb)), (name, b)
        sc = float(np.abs(rb).max())
        e = np.abs(gb - rb)
        if sc <= TINY:                                           # an exact zero of the reference, or a denormal gate's share
            ok = float(e.max()) <= TINY
            frac = 0.0
        else:
            frac = float(e.max()) / sc
            ok = e.max() <= GRAD_MAX * sc + TINY and (e.size < 16 or e.mean() <= GRAD_MEAN * sc + TINY)
        worst = max(worst, frac)
        if not ok:
            missed.append('%s row %d: max %.3e mean %.3e of its own max %.3e' % (name, b, frac, float(e.mean()) / max(sc, TINY), sc))
    line = 'gate extremes BPTT %s %s: worst regime at %.3e of its own max (bound %.1e)' % (tag, name, worst, GRAD_MAX)
    print(line); _tol_report(line)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('chain', ['wide', 'step'])
def test_bptt_with_prescribed_gates_matches_autograd(chain, shape, monkeypatch):
    """ops.fused_cell_train_with_gates on the gate table, loss = sum(H * R): d X, d h0, the three parameter gradients and BOTH gate
    gradients against fp64 autograd through the same recurrence. The gate gradients, d X and d h0 are held regime by regime to that
    regime's own magnitude: the derivative with respect to a gate that is 0 is not 0 (rows 1 - 4). Exactly: d X = 0 where gi = 0,
    d h0 = 0 where gf = 0."""
    from gated_gcrnns_amd import ops
    c, g = _case(shape), _case_grads(shape)
    _setenv(monkeypatch, CHAIN_ENV[chain])
    cell, Xd, hd, _, _, gi, gf = _device_case(c, torch.float32)      # fp32 master weights holding bf16-representable values
    for t_ in (Xd, hd, gi, gf):
        t_.requires_grad_(True)
    Rd = torch.tensor(c.R, dtype=torch.float32, device=Xd.device)
    spy = _spy(monkeypatch)
    H = ops.fused_cell_train_with_gates(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, gi, gf)
    (H.float() * Rd).sum().backward()
    ran = dict(spy.calls)
    assert ran.get(WIDE_CHAIN if chain == 'wide' else STEP_CHAIN, 0) >= 1 and ran.get(STEP_CHAIN if chain == 'wide' else WIDE_CHAIN, 0) == 0, ran
    err = np.abs(H.detach().double().cpu().numpy() - c.H).reshape(B, -1)
    assert err.max() <= _h_bounds(c)[0] and np.all(err.mean(axis=1) <= _h_bounds(c)[1])
    got = {'weight_A': cell.weight_A.grad, 'weight_B': cell.weight_B.grad, 'bias': cell.bias.grad, 'dX': Xd.grad, 'dh0': hd.grad, 'dgi': gi.grad, 'dgf': gf.grad}
    got = {k: v.double().cpu().numpy() for k, v in got.items()}
    missed = []
    tag = '%s chain N=%d' % (chain, c.N)
    pg = {k: g[k] for k in ('weight_A', 'weight_B', 'bias')}
    for k in pg:
        sc, tmax, tmean = _grad_scale_and_bounds(k, pg, GRAD_MAX, GRAD_MEAN)
        e = np.abs(got[k] - g[k])
        assert np.all(np.isfinite(got[k])), k
        line = 'gate extremes BPTT %s %s: max %.3e mean %.3e of its max (bounds %.1e / %.1e)' % (tag, k, e.max() / sc, e.mean() / sc, tmax, tmean)
        print(line); _tol_report(line)
        if not (e.max() <= tmax * sc and e.mean() <= tmean * sc):
            missed.append(line)
    _per_regime('dX', got['dX'], g['dX'], 0, missed, tag)
    _per_regime('dh0', got['dh0'], g['dh0'], 0, missed, tag)
    _per_regime('dgi', got['dgi'], g['dgi'], 1, missed, tag)
    _per_regime('dgf', got['dgf'], g['dgf'], 1, missed, tag)
    assert not missed, missed                                    # (every gradient is measured and reported before the first one fails the case)
    for b in X_DROPPED:
        assert float(np.abs(got['dX'][b]).max()) == 0.0, b
    for b in H_DROPPED:
        assert float(np.abs(got['dh0'][b]).max()) == 0.0, b
    assert float(np.abs(got['dh0'][RESET_ROW]).max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('chain', ['wide', 'step'])
def test_reset_step_cuts_the_bptt_chain_exactly(chain, shape, monkeypatch):
    """ops.fused_backward_data on the forward's own saved states with an upstream gradient that is zero on steps 0 - 1: behind a forget
    gate of exactly 0 at t = 2 nothing reaches dpre[0:2] or d h0 of the reset row (exact zeros) -- while the control row, same data,
    gate open, receives something. On the wide chain, ops.fused_backward_data_head on the factors (dy, w) of that upstream gradient gives
    the bits of ops.fused_backward_data on the materialised bf16(w (x) dy), with the table's forget gates (rows 2 and 11 included)."""
    from gated_gcrnns_amd import ops
    c = _case(shape)
    _setenv(monkeypatch, CHAIN_ENV[chain])
    cell, Xd, hd, _, _, gi, gf = _device_case(c, torch.float32)
    dev = Xd.device
    rng = np.random.default_rng(17)
    dy = torch.tensor(rng.standard_normal((B, T, c.N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    dy[:, :RESET_STEP] = 0
    w = torch.tensor(_head_weights(c.F), dtype=torch.float32, device=dev)
    dH = (dy.float().unsqueeze(2) * w.view(1, 1, c.F, 1)).to(torch.bfloat16).contiguous()
    wB, bias = cell.weight_B.detach().float(), cell.bias.detach().float()
    with torch.no_grad():
        hs_all, _, _ = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, return_states=True, gate_values=(gi, gf))
        hs, h0s = hs_all[1:], hs_all[:1]
        dHs, dHu = ops.fused_pack_upstream(dH, cell.graph, c.K)
        spy = _spy(monkeypatch)
        dpre, dh0, dgf = ops.fused_backward_data(dHs, hs, wB, cell.graph, want_dh0=True, gf=gf, h0s=h0s, bias=bias, dH_user=dHu)
        ran = dict(spy.calls)
        assert ran.get(WIDE_CHAIN if chain == 'wide' else STEP_CHAIN, 0) >= 1 and ran.get(STEP_CHAIN if chain == 'wide' else WIDE_CHAIN, 0) == 0, ran
        assert all(bool(torch.isfinite(a.float()).all()) for a in (dpre, dh0, dgf))
        assert float(dpre[:RESET_STEP, RESET_ROW, :c.N].float().abs().max()) == 0.0 and float(dh0[RESET_ROW, :c.N].float().abs().max()) == 0.0
        assert float(dpre[:RESET_STEP, 10, :c.N].float().abs().max()) > 0.0 and float(dh0[10, :c.N].float().abs().max()) > 0.0
        assert float(dpre[RESET_STEP:, RESET_ROW, :c.N].float().abs().max()) > 0.0
        for b in H_DROPPED:                                      # gf = 0 at every step: nothing is carried at all
            assert float(dpre[:RESET_STEP, b, :c.N].float().abs().max()) == 0.0 and float(dh0[b, :c.N].float().abs().max()) == 0.0
        if chain == 'wide':
            assert ops.fused_backward_data_head_plan(cell.graph, B, T, c.N, c.F, c.K) is not None
            got = ops.fused_backward_data_head(dy.contiguous(), w, hs, wB, cell.graph, want_dh0=True, gf=gf, h0s=h0s, bias=bias)
            for name, a_, b_ in zip(('dpre', 'dh0', 'dgf'), got, (dpre, dh0, dgf)):
                assert torch.equal(a_, b_), (name, int((a_ != b_).sum()))


# ------------------------------------------------------------------------------------------------------------ C. gates saturated by their own sub-networks
# (MLP_in.0.bias, MLP_forget.0.bias): after the fp32 sigmoid the gates are 0 (-120), ~1.8e-35 (-80), ~2.2e-29 (-66), exactly 1 (+120)
SAT_PAIRS = [(-120.0, 0.0), (0.0, -120.0), (-120.0, -120.0), (-80.0, 0.0), (-66.0, 120.0), (120.0, -66.0)]
DEAD_GRAD, DEAD_CEIL = 1e-25, 1e-20      # a reference gradient below DEAD_GRAD (g (1 - g) x an O(1e3) sum at g <= 2.2e-29) admits no relative
                                         # comparison: the kernel's must be finite and at most DEAD_CEIL in magnitude


def _cell_on(S, G, F, Kin, Kst, tg, seed):
    import gated_gcrnns_amd.Utils.graphML as gml
    torch.manual_seed(seed)
    cell = gml.GGCRNNCell(G, F, Kin, Kst, torch.tanh, tg, None, 1, True)
    cell.addGSO(torch.tensor(np.asarray(S)))
    return cell


def _reference(state, S, X, h0, R, tg):
    """fp64 states (numpy oracle) and gradients of loss = sum(H * R) (torch restatement under autograd; None where a parameter is unused)."""
    params = {k: v.double().numpy() for k, v in state.items()}
    H = orc.ggcrnn_cell(params, S, X, h0, tg)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    h0t = torch.tensor(h0, dtype=torch.float64, requires_grad=True)
    Ht = tref.ggcrnn_cell(P, torch.tensor(S, dtype=torch.float64), torch.tensor(X, dtype=torch.float64), h0t, tg)
    assert float((Ht.detach() - torch.tensor(H)).abs().max()) <= 1e-12
    (Ht * torch.tensor(R, dtype=torch.float64)).sum().backward()
    g = {k: (v.grad.numpy() if v.grad is not None else None) for k, v in P.items()}
    return H, g, h0t.grad.numpy()


def _set_state(cell, state):
    cell.load_state_dict(state)
    return cell


WGRAD_GATE_FLOOR = 1e-12         # the bf16 weight-gradient kernel leaves out an item whose gate is at or below this: with EVERY
                                 # item's gate below it the kernel's weight_A (weight_B) gradient is 0 where the reference's is g x an O(1e2) sum


def _check_grads(tag, cell, g, mx, mn, bf16_class, gate_range=None):
    """Every parameter gradient of `cell` against the reference's: bf16_class -> the class gates of tests/test_fused.py through
    _grad_scale_and_bounds (a scalar bias on its sibling weight's scale, as tests/test_directed_uniform.py does); otherwise mx of the gradient's own
    max. Gate sub-network gradients the reference has below DEAD_GRAD: finite and at most DEAD_CEIL; a main-cell gradient below TINY (weight_A under
    an input gate whose fp32 sigmoid is exactly 0): at most TINY. Everything else is compared relatively -- on the fp32-accurate and the
    small-graph paths weight_A under gi = 2.2e-29 included. gate_range (bf16 path): {'weight_A': (min, max) of gi over the items, 'weight_B': of
    gf}; where the max is at or below WGRAD_GATE_FLOOR the gradient may be off by the floor times the gradient an open gate would give, which
    max |reference| / min gate bounds from above."""
    is_dead = lambda k, v: float(np.abs(v).max()) < (DEAD_GRAD if k.startswith(('GFL_', 'MLP_')) else TINY)
    live = {k: v for k, v in g.items() if v is not None and not is_dead(k, v)}
    missed, worst, dead = [], (0.0, None), 0
    for k, q in cell.named_parameters():
        gr = g[k]
        got = None if q.grad is None else q.grad.double().cpu().numpy()
        if gr is None:                                           # (the unused output gate)
            assert got is None or float(np.abs(got).max()) == 0.0, k
            continue
        assert got is not None and np.all(np.isfinite(got)), k
        if k not in live:
            dead += 1
            assert float(np.abs(got).max()) <= (DEAD_CEIL if k.startswith(('GFL_', 'MLP_')) else TINY), (k, float(np.abs(got).max()))
            continue
        sc, tmax, tmean = float(np.abs(gr).max()), mx, mn
        if bf16_class and gr.size == 1 and k.endswith('.bias'):
            sib = k[:-5] + '.weight'
            sc = max(sc, float(np.abs(live[sib]).max()) if sib in live else 0.0)
        elif bf16_class:
            sc, tmax, tmean = _grad_scale_and_bounds(k, live, mx, mn)
        e = np.abs(got - gr)
        if gate_range is not None and k in gate_range and gate_range[k][1] <= WGRAD_GATE_FLOOR:
            assert float(e.max()) <= WGRAD_GATE_FLOOR * float(np.abs(gr).max()) / gate_range[k][0], (k, float(e.max()))
            dead += 1
            continue
        _tol_report('gate extremes %s %s max %.3e mean %.3e (bounds %.1e / %.1e)' % (tag, k, e.max() / sc, e.mean() / sc, tmax, tmean))
        if e.max() / sc > worst[0]:
            worst = (e.max() / sc, k)
        if not (e.max() <= tmax * sc and (e.size < 16 or e.mean() <= tmean * sc)):
            missed.append('%s max %.3e mean %.3e (bounds %.1e / %.1e)' % (k, e.max() / sc, e.mean() / sc, tmax, tmean))
    print('gate extremes %s: %d live gradients, worst %s at %.3e of its max (bound %.1e); %d dead ones <= %.0e' % (tag, len(live), worst[1], worst[0], mx, dead, DEAD_CEIL))
    assert not missed, (tag, missed)
    return dead


@functools.lru_cache(maxsize=None)
def _sat_case(shape, prec, pair):
    """A time-gated cell on the uniform-weight graph of test_wide._uniform_cell whose two gate read-outs carry the bias pair, and its fp64
    references; operands bf16- or fp32-representable (parameters bf16-representable in both)."""
    N, F, G, K = shape
    Bn, Tn = 2, 3
    cell, rng, S = _uniform_cell(N, G, F, K, SEED + 1 + N, time_gating=True)
    state = {k: v.detach().float().clone() for k, v in cell.state_dict().items()}
    state['MLP_in.0.bias'].fill_(pair[0]); state['MLP_forget.0.bias'].fill_(pair[1])
    rnd = bf16_round if prec == 'bf16' else f32_round
    X, h0, R = rnd(rng.standard_normal((Bn, Tn, G, N))), rnd(H0_STD * rng.standard_normal((Bn, F, N))), rnd(rng.standard_normal((Bn, Tn, F, N)))
    S32 = f32_round(S)
    H, g, dh0 = _reference(state, S32, X, h0, R, True)
    gi, gf = oracle_time_gates({k: v.double().numpy() for k, v in state.items()}, S32, X, h0)
    return types.SimpleNamespace(N=N, F=F, G=G, K=K, B=Bn, T=Tn, S=S, state=state, X=X, h0=h0, R=R, H=H, g=g, dh0=dh0, tg=True, sg=None,
                                 gate_range={'weight_A': (float(gi.min()), float(gi.max())), 'weight_B': (float(gf.min()), float(gf.max()))})


def _sat_device(c, dtype_x):
    dev = torch.device('cuda:0')
    cell = _set_state(_cell_on(c.S, c.G, c.F, c.K, c.K, True, 0), c.state).float().to(dev)      # fp32 (master) weights holding bf16-representable values
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).to(dtype_x)
    return cell, t(c.X), t(c.h0), torch.tensor(c.R, dtype=torch.float32, device=dev)


def test_saturating_biases_give_the_gates_the_issue_names():
    """CPU: the fp32 sigmoid of the six bias pairs -- 0, a normal float below the guard, one just above it, exactly 1."""
    s = lambda v: float(torch.sigmoid(torch.tensor(v, dtype=torch.float32)))
    assert s(-120.0) == 0.0 and s(120.0) == 1.0 and 1e-35 < s(-80.0) < 3e-35 and 1e-30 < s(-66.0) < 3e-29
    assert len(SAT_PAIRS) == 6


@pytest.mark.gpu
@pytest.mark.parametrize('pair', SAT_PAIRS)
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('gates_by', ['pair', 'each'])
def test_saturated_gate_subnetworks_bf16(gates_by, shape, pair, monkeypatch):
    """The bf16 fused path with its gates coming out of their own sub-networks saturated: inference and one training step, with the
    one-launch gate pair and with the per-gate pre-passes, against the fp64 oracle and the torch reference."""
    from gated_gcrnns_amd import ops
    c = _sat_case(shape, 'bf16', pair)
    monkeypatch.delenv('GCRNN_NO_GATE_PAIR', raising=False)
    _setenv(monkeypatch, {'GCRNN_SEQ32_MIN_B': '1'} if gates_by == 'pair' else {'GCRNN_SEQ32': '0', 'GCRNN_NO_GATE_PAIR': '1'})
    cell, Xd, hd, Rd = _sat_device(c, torch.bfloat16)
    mx, mn = _h_bounds(c)
    spy = _spy(monkeypatch)
    pair_entry, each_entries = 'gcrnn_fused_gate_pair_prepass_wide_bf16', ('gcrnn_fused_gate_prepass_bf16', 'gcrnn_fused_gate_prepass_pack_bf16')
    outs = []
    with torch.no_grad():
        assert cell._use_fused(Xd, hd)
        outs.append(('inference', cell(Xd, hd)))
    assert cell._use_fused_training(Xd, hd)
    H = cell(Xd, hd)
    (H.float() * Rd).sum().backward()
    outs.append(('training', H.detach()))
    ran = dict(spy.calls)
    if gates_by == 'pair':
        assert ran.get(pair_entry, 0) == 2 and sum(ran.get(n, 0) for n in each_entries) == 0, ran
    else:
        assert ran.get(pair_entry, 0) == 0 and sum(ran.get(n, 0) for n in each_entries) == 4, ran
    for what, Hk in outs:
        assert bool(torch.isfinite(Hk.float()).all())
        err = np.abs(Hk.double().cpu().numpy() - c.H)
        line = 'gate extremes saturated sub-networks %s bias %s gates by %s N=%d %s: |H - oracle| max %.3e mean %.3e (bounds %.1e / %.1e)' % (
            'bf16', pair, gates_by, c.N, what, err.max(), err.mean(), mx, mn)
        print(line); _tol_report(line)
        assert err.max() <= mx and err.mean() <= mn, (what, err.max(), err.mean())
    dead = _check_grads('saturated sub-networks bf16 bias %s gates by %s N=%d' % (pair, gates_by, c.N), cell, c.g, GRAD_MAX, GRAD_MEAN, True, c.gate_range)
    assert dead >= 5 * sum(1 for v in pair if v != 0.0)         # the saturated gates' own five parameters each


@pytest.mark.gpu
@pytest.mark.parametrize('pair', SAT_PAIRS)
def test_saturated_gate_subnetworks_fp32_accurate(pair, monkeypatch):
    """The same on the fp32-accurate path (ops.fused_cell_forward_x3_gated / fused_cell_train_x3_gated) at its own bounds: H to 1e-5,
    every live gradient to 2e-5 of its own max."""
    c = _sat_case(SMALL, 'f32', pair)
    cell, Xd, hd, Rd = _sat_device(c, torch.float32)
    spy = _spy(monkeypatch)
    with torch.no_grad():
        assert cell._use_fused_x3(Xd, hd, time_gated=True)
        Hi = cell(Xd, hd)
    assert sum(v for k, v in spy.calls.items() if k.startswith('gcrnn_fused_forward_x3')) >= 1, dict(spy.calls)
    assert cell._use_fused_x3_training(Xd, hd, time_gated=True)
    H = cell(Xd, hd)
    (H * Rd).sum().backward()
    for what, Hk in (('inference', Hi), ('training', H.detach())):
        e = float(np.abs(Hk.double().cpu().numpy() - c.H).max())
        line = 'gate extremes saturated sub-networks x3 bias %s %s: |H - oracle| max %.3e (bound 1e-5)' % (pair, what, e)
        print(line); _tol_report(line)
        assert bool(torch.isfinite(Hk).all()) and e <= 1e-5, (what, e)
    _check_grads('saturated sub-networks x3 bias %s' % (pair,), cell, c.g, 2e-5, 2e-5, False)


@functools.lru_cache(maxsize=None)
def _small_sat_case(N, K, pair):
    """The small-graph problem of test_small_graph_bptt_kernel_vs_composed_path (directed weighted graph, G = 1, F = 20) with the bias pair."""
    G, F, Bn, Tn = 1, 20, 3, 4
    rng = np.random.default_rng(N + Tn)
    S = rng.standard_normal((N, N)) * (rng.random((N, N)) < 0.08)
    S = (S / (np.abs(np.linalg.eigvals(S)).max() + 1e-9)).reshape(1, N, N)
    state = {k: v.detach().double().clone() for k, v in _cell_on(S, G, F, K, K, True, 0).state_dict().items()}
    state['MLP_in.0.bias'].fill_(pair[0]); state['MLP_forget.0.bias'].fill_(pair[1])
    state = {k: v.float().double() for k, v in state.items()}                   # fp32-representable: one reference serves both precisions
    X, h0, R = f32_round(rng.standard_normal((Bn, Tn, G, N))), f32_round(H0_STD * rng.standard_normal((Bn, F, N))), f32_round(rng.standard_normal((Bn, Tn, F, N)))
    H, g, dh0 = _reference(state, f32_round(S), X, h0, R, True)
    return types.SimpleNamespace(N=N, F=F, G=G, K=K, S=f32_round(S), state=state, X=X, h0=h0, R=R, H=H, g=g, dh0=dh0)


@pytest.mark.gpu
@pytest.mark.parametrize('pair', SAT_PAIRS)
@pytest.mark.parametrize('N,K', [(59, 3), (80, 5)])
@pytest.mark.parametrize('dt,tol,gtol', [(torch.float64, 1e-11, 1e-9), (torch.float32, 1e-5, 5e-4)])
def test_saturated_gate_subnetworks_small_graph(dt, tol, gtol, N, K, pair, monkeypatch):
    """ops.small_time_gates + ops.small_cell_train (one launch each way) in fp32 and fp64 at N = 59 and N = 80: states at the small-graph
    kernels' own bound, every live gradient (d h0 included) at the tolerance of test_small_graph_bptt_kernel_vs_composed_path."""
    from gated_gcrnns_amd import ops
    c = _small_sat_case(N, K, pair)
    dev = torch.device('cuda:0')
    cell = _set_state(_cell_on(c.S, c.G, c.F, c.K, c.K, True, 0).double(), c.state).to(dev).to(dt)
    Xd = torch.tensor(c.X, dtype=dt, device=dev)
    hd = torch.tensor(c.h0, dtype=dt, device=dev).requires_grad_(True)
    called = []
    for name in ('small_time_gates', 'small_cell_train'):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (called.append(n), f(*a, **k))[1])(getattr(ops, name), name))
    assert cell._use_small_training(Xd, hd)
    H = cell(Xd, hd)
    (H * torch.tensor(c.R, dtype=dt, device=dev)).sum().backward()
    assert called == ['small_time_gates', 'small_cell_train'], called
    e = float(np.abs(H.detach().double().cpu().numpy() - c.H).max())
    line = 'gate extremes saturated sub-networks small graph %s N=%d bias %s: |H - oracle| max %.3e (bound %.0e)' % (dt, N, pair, e, tol)
    print(line); _tol_report(line)
    assert bool(torch.isfinite(H).all()) and e <= tol, e
    _check_grads('saturated sub-networks small graph %s N=%d bias %s' % (dt, N, pair), cell, c.g, gtol, gtol, False)
    sc = float(np.abs(c.dh0).max())
    assert bool(torch.isfinite(hd.grad).all()) and float(np.abs(hd.grad.double().cpu().numpy() - c.dh0).max()) <= gtol * sc + TINY      # (both gates shut: 1e-51 in fp64)


# ------------------------------------------------------------------------------------------------------------ D. saturated states
SAT_BIAS = 100.0                  # 2 b = +-200 un-gated: the exp2 argument of the kernels' tanh (+-577) overflows / underflows


def _sat_features(F):
    return (1, F - 2), (3, F // 2 + 1)          # bias +100 / -100


def _isolate(S, nodes):
    S = np.array(S)
    for n in nodes:
        S[0, n, :] = 0.0
        S[0, :, n] = 0.0
    return S


@functools.lru_cache(maxsize=None)
def _state_case(shape, prec, tg, graph='uniform'):
    """Un-gated or time-gated cell (gates at their usual init) whose bias saturates four state features, on a graph with two nodes without
    neighbours, and its fp64 references. graph: 'uniform' (test_wide._uniform_cell's), 'small' (directed weighted, N <= 128), 'big'
    (tests/test_fused.random_graph beyond the fused kernels)."""
    from test_fused import random_graph
    N, F, G, K = shape
    Bn, Tn = 3, 3
    rng = np.random.default_rng(SEED + 2 + N)
    iso = (2, N - 3)
    if graph == 'uniform':
        S = _isolate(_uniform_cell(N, G, F, K, SEED + 2 + N)[2], iso)
    elif graph == 'small':
        S = rng.standard_normal((N, N)) * (rng.random((N, N)) < 0.08)
        S = _isolate((S / (np.abs(np.linalg.eigvals(S)).max() + 1e-9)).reshape(1, N, N), iso)
    else:
        S = _isolate(random_graph(N, 8.0 / N, 3), iso)
    assert not S[0, iso[0]].any() and not S[0, :, iso[1]].any()
    cell = _cell_on(S, G, F, K, K, tg, SEED + N)
    state = {k: v.detach().to(torch.bfloat16).float() for k, v in cell.state_dict().items()}
    plus, minus = _sat_features(F)
    assert len(set(plus + minus)) == 4
    state['bias'][list(plus)] = SAT_BIAS
    state['bias'][list(minus)] = -SAT_BIAS
    rnd = bf16_round if prec == 'bf16' else f32_round
    X, h0, R = rnd(rng.standard_normal((Bn, Tn, G, N))), rnd(H0_STD * rng.standard_normal((Bn, F, N))), rnd(rng.standard_normal((Bn, Tn, F, N)))
    S32 = f32_round(S)
    H, g, dh0 = _reference(state, S32, X, h0, R, tg)
    assert np.all(H[:, :, list(plus)] == 1.0) and np.all(H[:, :, list(minus)] == -1.0)          # the reference saturates exactly as well
    other = np.array([f for f in range(F) if f not in plus + minus])
    assert np.median(np.abs(H[:, :, other])) < 0.9                                                # ... and the other features are ordinary states
    return types.SimpleNamespace(N=N, F=F, G=G, K=K, B=Bn, T=Tn, S=S32, state=state, X=X, h0=h0, R=R, H=H, g=g, dh0=dh0, tg=tg, sg=None,
                                 plus=list(plus), minus=list(minus), other=other)


def _state_device(c, wdtype, xdtype):
    dev = torch.device('cuda:0')
    cell = _set_state(_cell_on(c.S, c.G, c.F, c.K, c.K, c.tg, 0), c.state).float().to(dev).to(wdtype)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).to(xdtype)
    return cell, t(c.X), t(c.h0), torch.tensor(c.R, dtype=torch.float32 if xdtype == torch.bfloat16 else xdtype, device=dev)


def _check_saturated(tag, H, c, mx, mn):
    """Exactly the sign on the saturated features at every node (the two without neighbours included), finite everywhere, the other
    features within the path's ordinary bound of the oracle."""
    Hn = H.detach().double().cpu().numpy()
    assert np.all(np.isfinite(Hn)), tag
    assert np.all(Hn[:, :, c.plus] == 1.0) and np.all(Hn[:, :, c.minus] == -1.0), tag
    err = np.abs(Hn[:, :, c.other] - c.H[:, :, c.other])
    line = 'gate extremes saturated states %s N=%d tg=%s: |H - oracle| on the other features max %.3e mean %.3e (bounds %.1e / %.1e)' % (
        tag, c.N, c.tg, err.max(), err.mean(), mx, mn)
    print(line); _tol_report(line)
    assert err.max() <= mx and err.mean() <= mn, (tag, err.max(), err.mean())


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('kernel', ['wide', 'seq16', 'step'])
def test_saturated_states_bf16_forward(kernel, shape, tg, monkeypatch):
    """bias = +-100 on four features: the bf16 forward kernels give exactly +-1 there (exp -> inf gives 1, exp -> 0 gives -1), no Inf / NaN,
    and the other features stay within the kernel's ordinary bound."""
    c = _state_case(shape, 'bf16', tg)
    _setenv(monkeypatch, FORWARD_ENV[kernel])
    cell, Xd, hd, _ = _state_device(c, torch.bfloat16, torch.bfloat16)
    spy = _spy(monkeypatch)
    with torch.no_grad():
        assert cell._use_fused(Xd, hd)
        H = cell(Xd, hd)
    ran = dict(spy.calls)
    wide = sum(ran.get(n, 0) for n in WIDE_ENTRIES) + ran.get('gcrnn_fused_forward_wide_user_bf16', 0)
    assert (wide == 1 and ran.get(STEP_ENTRY, 0) == 0) if kernel == 'wide' else (wide == 0 and ran.get(STEP_ENTRY, 0) == 1), ran
    _check_saturated(kernel, H, c, *_h_bounds(c))


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('shape', [SMALL, LARGE])
@pytest.mark.parametrize('chain', ['wide', 'step'])
def test_saturated_states_bf16_training(chain, shape, tg, monkeypatch):
    """One training step over the saturated features: every parameter gradient finite and within the bf16 class bounds of the torch
    reference (whose (1 - h^2) is exactly 0 there too), and -- read from ops.fused_backward_data on the step's own states -- dpre exactly 0
    on the saturated features at every node and step."""
    from gated_gcrnns_amd import ops
    c = _state_case(shape, 'bf16', tg)
    _setenv(monkeypatch, CHAIN_ENV[chain])
    cell, Xd, hd, Rd = _state_device(c, torch.float32, torch.bfloat16)
    spy = _spy(monkeypatch)
    assert cell._use_fused_training(Xd, hd)
    H = cell(Xd, hd)
    (H.float() * Rd).sum().backward()
    ran = dict(spy.calls)
    assert ran.get(WIDE_CHAIN if chain == 'wide' else STEP_CHAIN, 0) >= 1 and ran.get(STEP_CHAIN if chain == 'wide' else WIDE_CHAIN, 0) == 0, ran
    _check_saturated('training forward, %s chain' % chain, H, c, *_h_bounds(c))
    _check_grads('saturated states bf16 %s chain N=%d tg=%s' % (chain, c.N, tg), cell, c.g, GRAD_MAX, GRAD_MEAN, True)
    with torch.no_grad():
        hs = ops.to_sequence_major(H.detach(), cell.graph)
        dHs, dHu = ops.fused_pack_upstream(Rd.to(torch.bfloat16), cell.graph, c.K)
        gf = torch.full((c.T, c.B), 0.5, dtype=torch.float32, device=Xd.device) if tg else None
        dpre, dh0 = ops.fused_backward_data(dHs, hs, cell.weight_B.detach().float(), cell.graph, want_dh0=True, gf=gf, dH_user=dHu)
        sat = c.plus + c.minus
        assert bool(torch.isfinite(dpre[:, :, :c.N].float()).all()) and bool(torch.isfinite(dh0[:, :c.N].float()).all())
        assert float(dpre[:, :, :c.N][..., sat].float().abs().max()) == 0.0
        assert float(dpre[:, :, :c.N][..., c.other.tolist()].float().abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
def test_saturated_states_fp32_accurate(tg, monkeypatch):
    """The x3 forward (un-gated and time-gated) over the saturated features: exact signs, finite, the rest to 1e-5; one training step to
    2e-5 of each gradient's own max."""
    c = _state_case(SMALL, 'f32', tg)
    cell, Xd, hd, Rd = _state_device(c, torch.float32, torch.float32)
    spy = _spy(monkeypatch)
    with torch.no_grad():
        assert cell._use_fused_x3(Xd, hd, time_gated=tg)
        Hi = cell(Xd, hd)
    assert sum(v for k, v in spy.calls.items() if k.startswith('gcrnn_fused_forward_x3')) >= 1, dict(spy.calls)
    _check_saturated('x3 inference', Hi, c, 1e-5, 1e-5)
    assert cell._use_fused_x3_training(Xd, hd, time_gated=tg)
    H = cell(Xd, hd)
    (H * Rd).sum().backward()
    _check_saturated('x3 training forward', H, c, 1e-5, 1e-5)
    _check_grads('saturated states x3 tg=%s' % tg, cell, c.g, 2e-5, 2e-5, False)


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
@pytest.mark.parametrize('N,K', [(59, 3), (80, 5)])
def test_saturated_states_small_graph_fp32(N, K, tg):
    """The one-launch small-graph kernels in fp32 over the saturated features: inference and one training step."""
    c = _state_case((N, 20, 1, K), 'f32', tg, 'small')
    cell, Xd, hd, Rd = _state_device(c, torch.float32, torch.float32)
    with torch.no_grad():
        assert cell._use_small(Xd, hd)
        _check_saturated('small graph inference', cell(Xd, hd), c, 1e-5, 1e-5)
    hd.requires_grad_(True)
    assert cell._use_small_training(Xd, hd)
    H = cell(Xd, hd)
    (H * Rd).sum().backward()
    _check_saturated('small graph training forward', H, c, 1e-5, 1e-5)
    _check_grads('saturated states small graph N=%d tg=%s' % (N, tg), cell, c.g, 5e-4, 5e-4, False)
    assert bool(torch.isfinite(hd.grad).all()) and float(np.abs(hd.grad.double().cpu().numpy() - c.dh0).max()) <= 5e-4 * float(np.abs(c.dh0).max())


@pytest.mark.gpu
def test_saturated_states_bf16_streaming_path():
    """N = 1100 > 1024: bf16 inference in Horner form on the accumulate-SpMM (the shape and bounds of
    test_bf16_streaming_path_for_graphs_beyond_the_fused_kernel) over the saturated features."""
    c = _state_case((1100, 8, 8, 4), 'bf16', False, 'big')
    cell, Xd, hd, _ = _state_device(c, torch.bfloat16, torch.bfloat16)
    with torch.no_grad():
        assert not cell._use_fused(Xd, hd) and cell._use_horner(Xd, hd)
        H = cell(Xd, hd)
    _check_saturated('streaming Horner', H, c, 5e-2, 4e-3)
