"""The edge gate's softmax at its extremes, on each of its three implementations.

csrc/gcrnn_attention.hip (fp32 / fp64, two-pass; the composed path), csrc/gcrnn_edge_gate.hip (bf16 fused path: online softmax in chunks of eight
records, lean and HUB backward) and csrc/gcrnn_small_edge*.hip (fp32 / fp64, one workgroup per sequence). The rest of the suite draws its scores
from a fresh mixer or from 0.3 randn: no maximum that matters is subtracted, no running sum is rescaled over a large gap, no alpha is one-hot or
tied, and the LeakyReLU is never evaluated at exactly 0 (where its slope is the NEGATIVE one, 0.2, as nn.functional.leaky_relu has it).

A. Regime table (REGIMES / regime_scores): the scores s1[n] + s2[m] are PRESCRIBED, one regime per slice t (generic kernel, ops.edge_attention)
   or per item (fused kernels, where they are planted through two or three feature columns that a12 picks out), every regime on the same
   Wx / z and the same upstream gradient. Every sum is exact in fp32. Before any launch the CPU proves from the reference alone: at least 30 %
   of the rows of degree >= 2 are one-hot in the peak regimes and at least 10 % have tied winners; a row of degree > 8 has its maximum in its
   last chunk of eight records and one in its first; on the hub graph a row of more than 32 records has it beyond record 32; base / shift+ and
   basen / shift- agree; base, peak+ and flat0 are at least MARGIN = 20 bounds apart.
   Bounds: the generic kernel's 1e-12 (fp64) / 2e-5 (fp32) of each tensor's max (tests/test_hip_parity.py::test_edge_attention_kernels), per
   regime; the fused kernels' of tests/test_fused.py::test_fused_edge_attention_kernels_match_dense_autograd, per item: relu(o) <= 1/128 of the
   item's max, dz <= 1.5e-2 max / 2e-3 mean of the item's max, da_part <= 5e-3 of its max; padding rows exactly 0. The planted feature
   columns, whose magnitude is the scores', are held to their own max. A gradient of a regime that has VANISHED (below 1e-3 of the base
   regime's max of the same gradient) is held absolutely, to the bound times the base regime's max. ds2[m] sums the LeakyReLU slope times
   the softmax adjoint over row m, which is 0 wherever the row's entries that carry weight lie on one side of the kink (in this table: everywhere, base
   included): a vanished ds2 is held to the base regime's ds1 max, the same entries summed along the other index.
B. The edge-gated cell in the small-graph regime with zero / peaked mixers (tests/golden/g19_attention_regimes.npz for dir17, the torch
   reference for quake at T = 4), on the one-launch kernels (with and without the input gradient) and, under GCRNN_NO_SMALL_EDGE=1, on the
   composed path. fp64: 1e-11 on states, 1e-10 of each gradient's max. fp32, zero mixers: 1e-5 / 2e-5. fp32, peaked mixers: the mixers are
   the default initialisation times 2^12 (dir17) / 2^10 (quake), scores of magnitude 1e2 .. 1e4 carry fp32 rounding that the softmax
   amplifies, so the bound is max(standing, 8 x the error of oracle/torch_reference.py evaluated in torch float32 on the CPU against its own
   fp64): another order of summation than torch's, over T steps of the recurrence.

Two kernels changed with this file, each shown by one regime:
  shift- (generic, fp32): gcrnn_attention.hip formed slope * z at |z| ~ 5000 and then subtracted the row maximum: y, dWx, ds1 were 2.2e-5 .. 4.2e-5
    of their max off the reference (bound 2e-5). The exponent is now the difference of the scores times the slope wherever both lie on one
    side of the kink.
  the gated items (fused backward): gcrnn_edge_gate.hip rounded gate x upstream gradient to bf16 in its LDS image: da_part of single items was
    1.1e-3 .. 5.7e-3 of its max (bound 5e-3). The gate now scales the softmax adjoint and the gathered sum in fp32.
Besides, the LeakyReLU slope at a score of exactly 0 in gcrnn_small_edge*.hip and in the oracles (see tests/test_torch_reference.py, G19).

Measured on an MI355X (GCRNN_TOL_REPORT; worst case of each group next to its bound):
  A generic, worst regime of its own max: fp64 y 5.2e-14, dWx 5.8e-14, ds1 7.5e-14, ds2 2.0e-16 (1e-12); fp32 y 1.7e-7, dWx 2.7e-7, ds1 3.5e-7,
    ds2 1.1e-7 (2e-5); shift+ / base and shift- / basen, kernel against kernel: 0 in both precisions (twice the bound).
  A fused, worst item of the four cases: relu(o) 3.5e-3, planted columns 2.7e-3 (1/128); dz 3.3e-3 max, 1.1e-4 mean, planted columns 3.7e-3,
    1.7e-4 (1.5e-2 / 2e-3); da_part 2.8e-5, planted columns 3.1e-5 (5e-3), flat0 (the slope at the kink) 3.5e-7; padding rows exactly 0.
  B fp64, both cases, three settings, one-launch (with and without dX) and composed: states <= 2.7e-14 (1e-11), gradients <= 3.8e-13 (1e-10).
    fp32, zero mixers: states <= 6.7e-8 (1e-5), gradients <= 2.2e-6 (2e-5).
    fp32, peaked mixers: the torch reference in float32 on the CPU is off its own fp64 by 5.1e-7 (dir17) / 9.6e-6 (quake) on the states and by up
    to 3.3e-5 (dir17, forget mixer) / 1.1e-4 (quake, h0) on a gradient; the kernels: states 3.3e-7 / 5.9e-6, worst gradient 1.6e-5 (dir17, h0)
    / 8.8e-5 (quake, h0), every one at or below 0.26 of its bound max(standing, 8 x the reference's float32 error).
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import torch_reference as tr
from test_fused import _tol_report, bf16_round, random_graph
from test_hip_parity import _attention_torch
from test_small_edge_train import COMPOSED, TOLS, Tn, dev, gso_adj59, make_cell, new_path_only, spy      # noqa: F401  (fixtures)
from test_torch_reference import VANISHED, regime_grad_err

MARGIN = 20
REGIMES = ['flat0', 'flat+', 'flat-', 'base', 'shift+', 'basen', 'shift-', 'peak+', 'peak-', 'mixed']
R = {name: i for i, name in enumerate(REGIMES)}
SLOPE = 0.2
DX, BWD, FWD = 'gcrnn_small_edge_backward_dx', 'gcrnn_small_edge_backward', 'gcrnn_small_edge_forward'


def _report(line):
    print(line)
    _tol_report(line)


# ------------------------------------------------------------------------------------------------------------ A. the regime table
def support(S):
    """[m][n] support of the attention on the GSO S [1][N][N]: (S + I) != 0."""
    return np.abs(np.asarray(S, dtype=np.float64)[0] + np.eye(S.shape[1])) > tr.ZERO_TOLERANCE


def _winner_shares(mask, lvl):
    rows = np.nonzero(mask.sum(axis=1) >= 2)[0]
    winners = np.array([(lvl[mask[m]] == lvl[mask[m]].max()).sum() for m in rows])
    return float((winners == 1).mean()), float((winners >= 2).mean())


def node_tables(mask, seed, hub_row=None):
    """base1, base2 (integers in [-64, 64] / 16) and lvl (integers 0 .. 7), one per node. The levels are drawn with probabilities
    proportional to rho^level, rho the first of (1, 0.7, 0.5, 0.35, 0.25) at which this support has both unique and tied winners often enough
    (rows of two dozen records rarely have a unique maximum among eight equally likely levels). hub_row: that row's winner (level 7) is put at
    its record 40, with nothing above level 6 elsewhere in the row."""
    rng = np.random.default_rng(seed)
    N = mask.shape[0]
    base1, base2 = rng.integers(-64, 65, N) / 16.0, rng.integers(-64, 65, N) / 16.0
    for rho in (1.0, 0.7, 0.5, 0.35, 0.25):
        p = rho ** np.arange(8)
        lvl = rng.choice(8, N, p=p / p.sum())
        if hub_row is not None:
            cols = np.nonzero(mask[hub_row])[0]
            assert cols.size > 41
            lvl[cols] = np.minimum(lvl[cols], 6)
            lvl[cols[40]] = 7
        one, tied = _winner_shares(mask, lvl)
        if one >= 0.35 and tied >= 0.15:
            break
    return base1, base2, lvl


def regime_scores(base1, base2, lvl):
    """(s1, s2) [regime][node], fp64 holding fp32-exact values: the score of support entry (m, n) is s1[n] + s2[m]."""
    N = lvl.size
    z, o = np.zeros(N), np.ones(N)
    table = {'flat0': (z, z), 'flat+': (3 * o, 2 * o), 'flat-': (-3 * o, -2 * o), 'base': (base1 + 8, base2 + 8),
             'shift+': (base1 + 520, base2 + 520), 'basen': (base1 - 8, base2 - 8), 'shift-': (base1 - 2568, base2 - 2568),
             'peak+': (64.0 * lvl, o), 'peak-': (320.0 * (lvl - 8), -o), 'mixed': (64.0 * lvl - 256, base2)}
    s1 = np.stack([np.asarray(table[r][0], dtype=np.float64) for r in REGIMES])
    s2 = np.stack([np.asarray(table[r][1], dtype=np.float64) for r in REGIMES])
    return s1, s2


def assert_table_reaches_its_regimes(mask, s1, s2, lvl, hub_row=None):
    """CPU, from the table and the support alone."""
    for r in range(len(REGIMES)):                                           # exact in fp32: operands and every sum on the support
        a, b = s1[r].astype(np.float32), s2[r].astype(np.float32)
        assert np.array_equal(a.astype(np.float64), s1[r]) and np.array_equal(b.astype(np.float64), s2[r])
        z32 = (a[None, :] + b[:, None])[mask]
        assert np.array_equal(z32.astype(np.float64), (s1[r][None, :] + s2[r][:, None])[mask]), REGIMES[r]
    zb, zs = (s1[R['base']][None, :] + s2[R['base']][:, None])[mask], (s1[R['shift+']][None, :] + s2[R['shift+']][:, None])[mask]
    assert np.array_equal(zs - zb, np.full(zb.shape, 1024.0)) and zb.min() > 0
    zb, zs = (s1[R['basen']][None, :] + s2[R['basen']][:, None])[mask], (s1[R['shift-']][None, :] + s2[R['shift-']][:, None])[mask]
    assert np.array_equal(zs - zb, np.full(zb.shape, -5120.0)) and zb.max() < 0
    zm = (s1[R['mixed']][None, :] + s2[R['mixed']][:, None])[mask]
    assert (zm > 0).mean() > 0.1 and (zm < 0).mean() > 0.1
    deg = mask.sum(axis=1)
    one, tied = _winner_shares(mask, lvl)
    assert one >= 0.30 and tied >= 0.10 and lvl.min() >= 0 and lvl.max() == 7, (one, tied)
    first = {m: int(np.argmax(lvl[mask[m]])) for m in np.nonzero(deg > 8)[0]}          # position of the (first) maximum in the row's records
    assert any(p >= 8 * ((deg[m] - 1) // 8) for m, p in first.items()) and any(p < 8 for p in first.values())
    if hub_row is not None:
        assert deg[hub_row] > 32 and first[hub_row] > 32


def _per_regime_err(got, ref, base_ref=None):
    """max-abs error of one regime's tensor over the magnitude it is held to (its own max; a vanished gradient: the base regime's)."""
    own = float(ref.abs().max())
    scale = own
    if base_ref is not None and own < VANISHED * float(base_ref.abs().max()):
        scale = float(base_ref.abs().max())
    assert bool(torch.isfinite(got).all())
    return float((got.double() - ref).abs().max()) / (scale + 1e-300)


# -- generic kernel
GENERIC_SHAPES = [(80, 3, 5), (257, 2, 33)]


@functools.lru_cache(maxsize=None)
def _generic_case(N, B, F):
    """The graph of test_edge_attention_kernels (directed, weighted, an isolated node, a cancelled self-loop); ONE fp32-exact Wx and upstream
    gradient for every regime; the fp64 reference (values and gradients) on the CPU."""
    from gated_gcrnns_amd.graph import GraphOperator
    rng = np.random.default_rng(N)
    S = rng.standard_normal((N, N)) * (rng.random((N, N)) < 0.1)
    S[3, :] = 0; S[:, 3] = 0
    S[5, 5] = -1.0
    mask = support(S[None])
    assert mask[3].sum() == 1 and not mask[5, 5]
    base1, base2, lvl = node_tables(mask, N + 1)
    s1, s2 = regime_scores(base1, base2, lvl)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    Wx1, r1 = f32(rng.standard_normal((1, N, B, F))), f32(rng.standard_normal((1, N, B, F)))
    nR = len(REGIMES)
    Wx, r = np.repeat(Wx1, nR, axis=0), np.repeat(r1, nR, axis=0)
    S1, S2 = np.repeat(s1[:, :, None], B, axis=2), np.repeat(s2[:, :, None], B, axis=2)
    graph = GraphOperator(S[None])
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (Wx, S1, S2)]
    y = _attention_torch(t[0], t[1], t[2], graph, SLOPE)
    (y * torch.tensor(r)).sum().backward()
    ref = [y.detach()] + [a.grad for a in t]
    return types.SimpleNamespace(S=S, mask=mask, lvl=lvl, s1=s1, s2=s2, Wx=Wx, S1=S1, S2=S2, r=r, ref=ref)


@pytest.mark.parametrize('N,B,F', GENERIC_SHAPES)
def test_regime_table_on_the_generic_graphs_cpu(N, B, F):
    c = _generic_case(N, B, F)
    assert_table_reaches_its_regimes(c.mask, c.s1, c.s2, c.lvl)
    y = c.ref[0]
    assert bool(all(torch.isfinite(a).all() for a in c.ref))
    tol = 2e-5 * float(y.abs().max())
    assert float((y[R['shift+']] - y[R['base']]).abs().max()) <= 1e-12 and float((y[R['shift-']] - y[R['basen']]).abs().max()) <= 1e-12
    for a, b in (('base', 'peak+'), ('base', 'flat0'), ('peak+', 'flat0'), ('basen', 'peak-')):
        assert float((y[R[a]] - y[R[b]]).abs().max()) >= MARGIN * tol, (a, b)
    assert float(c.ref[2][R['flat0']].abs().max()) > 1e-2                   # the kink is live: ds1 of flat0 is not 0
    # ds2[m] sums slope x (softmax adjoint) over row m: 0 wherever the entries of a row that carry weight lie on one side of the kink
    assert float(c.ref[3][R['base']].abs().max()) <= 1e-12 and float(c.ref[3][R['flat-']].abs().max()) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize('dt,tol', [(torch.float64, 1e-12), (torch.float32, 2e-5)])
@pytest.mark.parametrize('N,B,F', GENERIC_SHAPES)
def test_generic_attention_kernels_at_the_softmax_extremes(dev, dt, tol, N, B, F):
    """gcrnn_attention_forward / _backward, one regime per slice t, against the fp64 index-op restatement: y, dWx, ds1, ds2 per regime; the
    shifted regimes against their unshifted twins, kernel against kernel, within twice the bound."""
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator
    c = _generic_case(N, B, F)
    assert_table_reaches_its_regimes(c.mask, c.s1, c.s2, c.lvl)
    graph = GraphOperator(c.S[None], device=dev)
    Wx, s1, s2 = (torch.tensor(a, dtype=dt, device=dev).requires_grad_(True) for a in (c.Wx, c.S1, c.S2))
    y = ops.edge_attention(Wx, s1, s2, graph)
    (y * torch.tensor(c.r, dtype=dt, device=dev)).sum().backward()
    got = [a.detach().cpu() for a in (y, Wx.grad, s1.grad, s2.grad)]
    missed = []
    for name, g, ref, rel_base in zip(('y', 'dWx', 'ds1', 'ds2'), got, c.ref, (False, False, True, True)):
        errs = [_per_regime_err(g[i], ref[i], c.ref[2][R['base']] if rel_base else None) for i in range(len(REGIMES))]
        _report('attention regimes generic %s N=%d %s: worst regime %s at %.3e of its max (bound %.0e); per regime %s' % (
            dt, N, name, REGIMES[int(np.argmax(errs))], max(errs), tol, ' '.join('%.1e' % e for e in errs)))
        missed += ['%s %s %.3e' % (name, REGIMES[i], e) for i, e in enumerate(errs) if e > tol]
        for a, b in (('shift+', 'base'), ('shift-', 'basen')):
            sc = float((c.ref[2] if rel_base else ref)[R[b]].abs().max())
            e = float((g[R[a]].double() - g[R[b]].double()).abs().max()) / sc
            _report('attention regimes generic %s N=%d %s: %s against %s, kernel against kernel, %.3e (bound %.0e)' % (dt, N, name, a, b, e, 2 * tol))
            if e > 2 * tol:
                missed.append('%s %s vs %s %.3e' % (name, a, b, e))
    assert not missed, missed


# -- fused bf16 kernels
P1, P2, PC = 1, 2, 3                       # planted feature columns: s1 = z[:, P1] (+ shift), s2 = z[:, P2] (+ shift), z[:, PC] = 1 carries the shift
PLANTED = [P1, P2, PC]
GROUPS = [(0.0, ['flat0', 'flat+', 'flat-', 'base', 'basen', 'peak+', 'peak-', 'mixed']), (512.0, ['base', 'shift+']), (-2560.0, ['basen', 'shift-'])]
FUSED_CASES = {'plain64': (200, 64, False, False), 'hub64': (200, 64, True, False), 'plain32': (200, 32, False, False), 'gated32': (200, 32, False, True)}
HUB_ROW, HUB_COL, HUB_DEG = 7, 11, 60


@functools.lru_cache(maxsize=None)
def _fused_graph(N, hub):
    S = random_graph(N, 10.0 / N, 83)[0].copy()
    if hub:
        rng = np.random.default_rng(84)
        S[HUB_ROW, :HUB_DEG] = rng.uniform(0.05, 0.3, HUB_DEG)
        S[:HUB_DEG, HUB_COL] = rng.uniform(0.05, 0.3, HUB_DEG)
    S = S.astype(np.float32).astype(np.float64).reshape(1, N, N)
    mask = support(S)
    base1, base2, lvl = node_tables(mask, 85, HUB_ROW if hub else None)
    return S, mask, base1, base2, lvl


def _planted_items(shift, names, z0, base1, base2, lvl):
    """z [items][N][F] and a12 [2][F] of one launch: the regimes `names` with the constant column weighted by `shift`. With a shift the
    table's base / basen rows are planted and the shift turns them into shift+ / shift- (the unshifted twin, under a zero weight, rides along)."""
    s1, s2 = regime_scores(base1, base2, lvl)
    F = z0.shape[1]
    z = np.repeat(z0[None], len(names), axis=0)
    for i, name in enumerate(names):
        src = {'shift+': 'base', 'shift-': 'basen'}.get(name, name)
        z[i, :, P1], z[i, :, P2], z[i, :, PC] = s1[R[src]], s2[R[src]], 1.0 if name.startswith('shift') else 0.0
    a12 = np.zeros((2, F))
    a12[0, P1] = a12[1, P2] = 1.0
    a12[0, PC] = a12[1, PC] = shift
    assert np.array_equal(bf16_round(z), z) and np.array_equal(bf16_round(a12), a12)
    return z, a12


def _dense_reference(z, a12, S, dpre, g):
    """The dense fp64 restatement of tests/test_fused.py (graphML.py:585-627 + ReLU) with a12 expanded per item: r, dz, da [items][2][F]."""
    items, N, F = z.shape
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(np.repeat(a12[None], items, axis=0), dtype=torch.float64, requires_grad=True)
    Sp = torch.tensor(S[0]) + torch.eye(N, dtype=torch.float64)
    mask = Sp.abs() > 1e-9
    s1, s2 = torch.einsum('inf,if->in', zt, at[:, 0]), torch.einsum('inf,if->in', zt, at[:, 1])
    e = torch.nn.functional.leaky_relu(s1[:, None, :] + s2[:, :, None], SLOPE).masked_fill(~mask, float('-inf'))
    alpha = torch.where(mask, torch.softmax(e, dim=2), torch.zeros((), dtype=torch.float64))
    r = torch.relu(torch.einsum('imn,imf->inf', alpha * Sp, zt))
    (r * torch.tensor(dpre) * torch.tensor(g)[:, None, None]).sum().backward()
    return r.detach(), zt.grad, at.grad, (s1.detach()[:, None, :] + s2.detach()[:, :, None])


@functools.lru_cache(maxsize=None)
def _fused_case(name):
    N, F, hub, gated = FUSED_CASES[name]
    S, mask, base1, base2, lvl = _fused_graph(N, hub)
    rng = np.random.default_rng(31 + F)
    z0 = bf16_round(rng.standard_normal((N, F)))
    dpre1 = bf16_round(rng.standard_normal((N, F)))
    launches = []
    for shift, names in GROUPS:
        z, a12 = _planted_items(shift, names, z0, base1, base2, lvl)
        dpre = np.repeat(dpre1[None], len(names), axis=0)
        g = rng.uniform(0.3, 1.0, len(names)).astype(np.float32).astype(np.float64) if gated else np.ones(len(names))
        r, dz, da, scores = _dense_reference(z, a12, S, dpre, g)
        launches.append(types.SimpleNamespace(shift=shift, names=names, z=z, a12=a12, dpre=dpre, g=g, r=r, dz=dz, da=da, scores=scores))
    return types.SimpleNamespace(N=N, F=F, hub=hub, gated=gated, S=S, mask=mask, lvl=lvl, base1=base1, base2=base2, launches=launches)


def _split_err(got, ref):
    """(error of the planted columns over their own max, error of the other columns over theirs), one item [N][F]."""
    other = [f for f in range(ref.shape[1]) if f not in PLANTED]
    e = (got.double() - ref).abs()
    sp, so = float(ref[:, PLANTED].abs().max()), float(ref[:, other].abs().max())
    ep = float(e[:, PLANTED].max()) / sp if sp > 0 else float(e[:, PLANTED].max())
    return ep, float(e[:, other].max()) / so, float(e[:, other].mean()) / so, float(e[:, PLANTED].mean()) / sp if sp > 0 else 0.0


def _da_err(got, ref, z, base_other):
    """da_part [2][F] of one item: (error of the columns that are not planted over their max -- vanished: over the base item's --, error of
    the planted columns over their scale). da[.][f] = sum_n ds[n] z[n][f] is linear in column f of z, and so is its rounding error, which is
    relative to sum |ds| |z|, not to the sum: in the peak regimes the planted columns' sums are 0 (tied winners share their level, and the
    softmax adjoint sums to 0 over them) while their terms are 1e3 times the others'. Their scale is the larger of their own max and the
    other columns' scale times max |z planted| / max |z other|."""
    other = [f for f in range(ref.shape[1]) if f not in PLANTED]
    e = (got.double() - ref).abs()
    own = float(ref[:, other].abs().max())
    so = own if own >= VANISHED * base_other else base_other
    sp = max(float(ref[:, PLANTED].abs().max()), so * float(np.abs(z[:, PLANTED]).max()) / float(np.abs(z[:, other]).max()))
    ep = float(e[:, PLANTED].max())
    return float(e[:, other].max()) / so, (ep / sp if sp > 0 else ep), so == own


@pytest.mark.parametrize('name', sorted(FUSED_CASES))
def test_regime_table_planted_in_the_fused_items_cpu(name):
    """CPU: the planted scores ARE the table's (exactly, also as an fp32 sum over the features in any order: every other a12 entry is 0), the
    table reaches its regimes on this graph, every regime is finite in the reference, the shifted items repeat their twins, and base / peak+ /
    flat0 differ by at least 20 bounds on the columns that are not planted."""
    c = _fused_case(name)
    s1, s2 = regime_scores(c.base1, c.base2, c.lvl)
    assert_table_reaches_its_regimes(c.mask, s1, s2, c.lvl, HUB_ROW if c.hub else None)
    deg_out, deg_in = c.mask.sum(axis=1), c.mask.sum(axis=0)
    assert (deg_out.max() > 32) == c.hub and (deg_in.max() > 32) == c.hub
    for L in c.launches:
        for i, nm in enumerate(L.names):
            want = s1[R[nm]][None, :] + s2[R[nm]][:, None]
            assert np.array_equal(L.scores[i].numpy()[c.mask], want[c.mask]), nm
            assert np.count_nonzero(L.a12) <= 4
        assert bool(torch.isfinite(L.r).all() and torch.isfinite(L.dz).all() and torch.isfinite(L.da).all())
        if L.shift:
            other = [f for f in range(c.F) if f not in PLANTED]
            assert float((L.r[0][:, other] - L.r[1][:, other]).abs().max()) <= 1e-12
    A = c.launches[0]
    other = [f for f in range(c.F) if f not in PLANTED]
    ro = A.r[:, :, other]
    tol = float(ro.abs().max()) / 128
    ix = {n: i for i, n in enumerate(A.names)}
    for a, b in (('base', 'peak+'), ('base', 'flat0'), ('peak+', 'flat0')):
        d = float((ro[ix[a]] - ro[ix[b]]).abs().max())
        assert d >= MARGIN * tol, (a, b, d, tol)
    assert float(A.da[ix['flat0']].abs().max()) > 1e-2                      # the kink is live


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FUSED_CASES))
def test_fused_attention_kernels_at_the_softmax_extremes(name):
    """gcrnn_fused_edge_attention_bf16 and its backward (lean; HUB on the hub graph), one regime per item, three launches (one per a12),
    against the dense fp64 restatement on the same bf16-representable operands, item by item."""
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import as_operator
    c = _fused_case(name)
    dev = torch.device('cuda:0')
    graph = as_operator(torch.tensor(c.S)).to(dev)
    npad = graph.fused_plan()['npad']
    N, F = c.N, c.F
    assert ops.lib.gcrnn_fused_edge_attention_supported(N, F) == 1
    assert (graph.edge_plan()['max_out_degree'] > 32) == c.hub
    assert ops.lib.gcrnn_fused_edge_attention_backward_supported(N, F, int(graph.edge_plan()['max_out_degree'])) == 1
    missed = []
    for L in c.launches:
        items = len(L.names)
        zd = torch.zeros((items, npad, F), dtype=torch.bfloat16, device=dev)
        zd[:, :N] = torch.tensor(L.z, dtype=torch.bfloat16, device=dev)
        dd = torch.zeros_like(zd)
        dd[:, :N] = torch.tensor(L.dpre, dtype=torch.bfloat16, device=dev)
        a12d = torch.tensor(L.a12, dtype=torch.float32, device=dev)
        gd = torch.tensor(L.g, dtype=torch.float32, device=dev) if c.gated else None
        r = ops.fused_edge_attention(zd, a12d, graph, N=N, negative_slope=SLOPE)
        dz, da_part, dgate = ops.fused_edge_attention_backward(dd, r, gd, zd, a12d, graph, N, negative_slope=SLOPE)
        torch.cuda.synchronize()
        r, dz, da_part = r.cpu(), dz.cpu(), da_part.cpu()
        assert bool(torch.isfinite(r.float()).all() and torch.isfinite(dz.float()).all() and torch.isfinite(da_part).all())
        if npad > N:
            assert float(r[:, N:].float().abs().max()) == 0.0 and float(dz[:, N:].float().abs().max()) == 0.0
        other = [f for f in range(F) if f not in PLANTED]
        base_da = float(L.da[L.names.index('base' if 'base' in L.names else 'basen')][:, other].abs().max())
        for i, nm in enumerate(L.names):
            tag = 'attention regimes fused %s shift %g %s' % (name, L.shift, nm)
            ep, eo, _, _ = _split_err(r[i, :N], L.r[i])
            _report('%s: relu(o) %.3e of its max, planted columns %.3e of theirs (bound %.1e)' % (tag, eo, ep, 1.0 / 128))
            if max(ep, eo) > 1.0 / 128:
                missed.append('%s relu(o) %.3e / %.3e' % (tag, eo, ep))
            ep, eo, mo, mp = _split_err(dz[i, :N], L.dz[i])
            _report('%s: dz max %.3e mean %.3e of its max, planted columns %.3e / %.3e of theirs (bounds 1.5e-2 / 2e-3)' % (tag, eo, mo, ep, mp))
            if max(ep, eo) > 1.5e-2 or max(mo, mp) > 2e-3:
                missed.append('%s dz %.3e %.3e / %.3e %.3e' % (tag, eo, mo, ep, mp))
            eo, ep, own = _da_err(da_part[i], L.da[i], L.z[i], base_da)
            _report('%s: da_part %.3e of %s max, planted columns %.3e of their scale (bound 5e-3)' % (tag, eo, 'its' if own else "the base item's", ep))
            if max(eo, ep) > 5e-3:
                missed.append('%s da_part %.3e / %.3e' % (tag, eo, ep))
        if c.gated:
            dg_ref = (r[:, :N].double() * torch.tensor(L.dpre)).sum(dim=(1, 2))
            assert float((dgate.double().cpu() - dg_ref).abs().max()) <= 1e-4 * float(dg_ref.abs().max()) + 1e-4
    assert not missed, missed


# ------------------------------------------------------------------------------------------------------------ B. the small-graph cell
SETTINGS = ['zero_zero', 'peaked_peaked', 'zero_peaked']
PEAK_K = {}                                # case -> the power of two its peaked mixers are the default initialisation times (filled by _cell_case)
ATT = ('input_attention', 'forget_attention')


def _one_hot_shares(params, S, X, h0):
    """Share of the support rows of two or more entries whose largest alpha is >= 1 - 1e-6, for the input and the forget attention, over
    every step; from oracle/torch_reference.py alone."""
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    St, Xt, ht = torch.tensor(S), torch.tensor(X), torch.tensor(h0)
    H = tr.ggcrnn_cell(P, St, Xt, ht, False, 'edge')
    mask = torch.tensor(support(S))
    rows = mask.sum(dim=1) >= 2
    out = []
    for att, w, seq in ((ATT[0], P['weight_A'], [Xt[:, t] for t in range(X.shape[1])]), (ATT[1], P['weight_B'], [ht] + [H[:, t] for t in range(X.shape[1] - 1)])):
        u = torch.cat([tr.lsigf(w, St, v, P.get('bias')) for v in seq], dim=0)
        F = u.shape[1]
        Wx = torch.einsum('fg,bgn->bfn', P[att + '.weight'][0, 0], u)
        a = P[att + '.mixer'][0, 0]
        z = torch.einsum('f,bfn->bn', a[:F], Wx)[:, None, :] + torch.einsum('f,bfn->bn', a[F:], Wx)[:, :, None]
        e = torch.nn.functional.leaky_relu(z, SLOPE).masked_fill(~mask, float('-inf'))
        top = torch.softmax(e[:, rows], dim=2).max(dim=2).values
        out.append(float((top >= 1 - 1e-6).double().mean()))
    return out


def _tr_run(params, S, X, h0, Rw, dtype):
    """oracle/torch_reference.py on the CPU in `dtype`, loss (H * Rw).sum(): (H, {parameter, 'h0', 'X': gradient}), all as fp64 tensors."""
    P = {k: torch.tensor(v, dtype=torch.float64).to(dtype).requires_grad_() for k, v in params.items()}
    Xt, ht = (torch.tensor(a, dtype=torch.float64).to(dtype).requires_grad_() for a in (X, h0))
    H = tr.ggcrnn_cell(P, torch.tensor(S, dtype=torch.float64).to(dtype), Xt, ht, False, 'edge')
    (H * torch.tensor(Rw, dtype=torch.float64).to(dtype)).sum().backward()
    g = {k: v.grad.double() for k, v in P.items()}
    g.update(h0=ht.grad.double(), X=Xt.grad.double())
    return H.detach().double(), g


def _with_mixers(params, default, setting, k):
    p = dict(params)
    for att, kind in zip(ATT, setting.split('_')):
        p[att + '.mixer'] = {'zero': 0.0, 'peaked': k, 'default': 1.0}[kind] * default[att + '.mixer']
    return p


@functools.lru_cache(maxsize=None)
def _cell_case(name, setting):
    """(cell shape, S, X, h0, R, parameters, reference H, reference gradients, the default-init regime's gradients, the error of the torch
    reference in float32 against them): dir17 from the reference's own fixture, quake (cut to T = 4) from the torch reference."""
    if name == 'dir17':
        g = load_golden('g19_attention_regimes')
        S, X, h0, Rw = g['S'], g['cell_X'], g['cell_h0'], g['cell_R']
        shape = (3, 7, 3, 2)
        params = g['cell_%s_params' % setting]
        Href, gref = torch.tensor(g['cell_%s_H' % setting]), {k: torch.tensor(v) for k, v in g['cell_%s_grads' % setting].items()}
        gdef = {k: torch.tensor(v) for k, v in g['cell_default_default_grads'].items()}
        PEAK_K[name] = float(g['cell_k'])
    else:
        S = gso_adj59()
        G, F, K, T, B = 1, 20, 4, 4, 3
        shape = (G, F, K, K)
        rng = np.random.default_rng(594)
        X, h0, Rw = rng.standard_normal((B, T, G, 59)), np.tanh(rng.standard_normal((B, F, 59))), rng.standard_normal((B, T, F, 59))
        default = {k: v.detach().numpy().copy() for k, v in make_cell(S, G, F, K, K, False, True, seed=63).state_dict().items()}
        if name not in PEAK_K:
            k = 1.0
            while (min(_one_hot_shares(_with_mixers(default, default, 'peaked_peaked', k), S, X, h0)) < 0.30
                   or _one_hot_shares(_with_mixers(default, default, 'zero_peaked', k), S, X, h0)[1] < 0.30):
                k *= 2.0
                assert k <= 2.0 ** 20
            PEAK_K[name] = k
        params = _with_mixers(default, default, setting, PEAK_K[name])
        Href, gref = _tr_run(params, S, X, h0, Rw, torch.float64)
        gdef = _tr_run(default, S, X, h0, Rw, torch.float64)[1] if setting != 'default_default' else gref
    H32, g32 = _tr_run(params, S, X, h0, Rw, torch.float32)
    cpu32 = {k: regime_grad_err(g32[k], gref[k].numpy(), gdef[k].numpy()) for k in gref}
    cpu32['H'] = float((H32 - Href).abs().max())
    return types.SimpleNamespace(shape=shape, S=S, X=X, h0=h0, Rw=Rw, params=params, Href=Href, gref=gref, gdef=gdef, cpu32=cpu32)


@pytest.mark.parametrize('name', ['dir17', 'quake'])
def test_cell_settings_reach_the_regimes_cpu(name):
    """CPU: zero mixers give scores of exactly 0 (alpha = 1 / degree), the peaked ones at least 30 % one-hot rows in each peaked gate, on the
    torch reference alone; the reference's gradient w.r.t. a zero mixer is not 0; the peaked settings' states differ from the zero ones'."""
    c0, cp, cz = (_cell_case(name, s) for s in SETTINGS)
    assert all(float(np.abs(c0.params[a + '.mixer']).max()) == 0.0 for a in ATT) and float(np.abs(cz.params[ATT[0] + '.mixer']).max()) == 0.0
    assert min(_one_hot_shares(cp.params, cp.S, cp.X, cp.h0)) >= 0.30 and _one_hot_shares(cz.params, cz.S, cz.X, cz.h0)[1] >= 0.30
    assert max(_one_hot_shares(c0.params, c0.S, c0.X, c0.h0)) == 0.0
    assert all(float(c0.gref[a + '.mixer'].abs().max()) > 1e-3 for a in ATT)
    assert float((c0.Href - cp.Href).abs().max()) > 0.1 and float((c0.Href - cz.Href).abs().max()) > 0.1
    print('attention regimes cell %s: peaked mixers = default x %g; torch float32 against fp64 on the CPU: %s' % (
        name, PEAK_K[name], {s: {k: float('%.2e' % v) for k, v in _cell_case(name, s).cpu32.items()} for s in SETTINGS}))


def _run_cell(c, dt, dev, x_grad):
    G, F, Kin, Kst = c.shape
    cell = make_cell(c.S, G, F, Kin, Kst, False, True, seed=0)
    cell.load_state_dict({k: torch.tensor(v) for k, v in c.params.items()})
    cell = copy.deepcopy(cell).to(dev).to(dt)
    Xd, hd = Tn(c.X, dt, dev).requires_grad_(x_grad), Tn(c.h0, dt, dev).requires_grad_()
    H = cell(Xd, hd)
    (H * Tn(c.Rw, dt, dev)).sum().backward()
    grads = {k: p.grad for k, p in cell.named_parameters() if p.grad is not None}
    grads['h0'] = hd.grad
    if x_grad:
        grads['X'] = Xd.grad
    return H.detach(), grads


def _check_cell(tag, c, H, grads, dt, peaked, expect, missed):
    tol_h, tol_g = TOLS[dt]
    amplified = dt == torch.float32 and peaked
    bound_h = max(tol_h, 8 * c.cpu32['H']) if amplified else tol_h
    assert bool(torch.isfinite(H).all())
    e = float((H.double().cpu() - c.Href).abs().max())
    _report('%s: states max-abs %.3e (bound %.3e)' % (tag, e, bound_h))
    if e > bound_h:
        missed.append('%s states %.3e > %.3e' % (tag, e, bound_h))
    assert expect <= set(grads), sorted(expect - set(grads))
    worst = (0.0, None, 0.0)
    for k in sorted(expect):
        bound = max(tol_g, 8 * c.cpu32[k]) if amplified else tol_g
        e = regime_grad_err(grads[k], c.gref[k].numpy(), c.gdef[k].numpy())
        if e / bound > worst[0]:
            worst = (e / bound, k, e)
        if e > bound:
            missed.append('%s grad %s %.3e > %.3e' % (tag, k, e, bound))
    _report('%s: worst gradient %s at %.3e of its scale, %.2f of its bound' % (tag, worst[1], worst[2], worst[0]))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [torch.float64, torch.float32])
@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('name', ['dir17', 'quake'])
def test_small_graph_edge_cell_at_zero_and_peaked_mixers(dev, spy, monkeypatch, name, setting, dt):
    """The one-launch kernels (gcrnn_small_edge_forward + _backward; + _backward_dx when X wants a gradient) and then the composed path
    (gcrnn_attention_*) on the same cell: states and every gradient, zero mixers at the standing bounds (the slope at the kink decides the
    mixer gradients there), peaked ones in fp32 at max(standing, 8 x the torch reference's own float32 error)."""
    c = _cell_case(name, setting)
    peaked = 'peaked' in setting
    names = set(c.gref) - {'X'}
    missed = []
    tag = 'attention regimes cell %s %s %s' % (name, setting, str(dt).split('.')[1])
    H, grads = _run_cell(c, dt, dev, False)
    new_path_only(spy)
    assert spy.calls[FWD] == 1 and spy.calls[DX] == 0
    _check_cell(tag + ' one-launch', c, H, grads, dt, peaked, names, missed)
    monkeypatch.setenv('GCRNN_SMALL_EDGE_DX', '1')                           # (an X that wants a gradient takes the one-launch path only with it)
    H, grads = _run_cell(c, dt, dev, True)
    assert spy.calls[DX] == 1 and spy.calls[BWD] == 1 and spy.calls[FWD] == 2 and all(spy.calls[n] == 0 for n in COMPOSED), dict(spy.calls)
    _check_cell(tag + ' one-launch with dX', c, H, grads, dt, peaked, names | {'X'}, missed)
    monkeypatch.delenv('GCRNN_SMALL_EDGE_DX')
    monkeypatch.setenv('GCRNN_NO_SMALL_EDGE', '1')
    H, grads = _run_cell(c, dt, dev, False)
    assert spy.calls[BWD] == 1 and spy.calls[DX] == 1 and spy.calls[FWD] == 2 and spy.calls['gcrnn_attention_backward'] > 0, dict(spy.calls)
    _check_cell(tag + ' composed', c, H, grads, dt, peaked, names, missed)
    assert not missed, missed
