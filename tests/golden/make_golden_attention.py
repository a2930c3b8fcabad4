#!/usr/bin/env python3
"""Generate the G19 golden vectors (the edge gate's softmax at its extremes) from the IMPORTED reference (build container only).

    python tests/golden/make_golden_attention.py          # needs the reference checkout (GCRNN_REFERENCE)

Same recipe as make_golden.py: the reference is imported read-only, run on CPU in float64, and only data is stored. One file,
g19_attention_regimes.npz, on the 17-node directed graph of tests/test_small_edge_train.py::gso_dir17 (an empty support row, an isolated
node, a hub row):

  att_<regime>/{x, a, W, y, grad_x, grad_a, grad_W}   graphAttention (G = 3, F = 7, B = 2, one head), loss sum(y * att_R), for the mixers
      zero      a = 0: every score is exactly 0 (the LeakyReLU's kink), alpha = 1 / degree
      default   the default initialisation (the magnitude that vanishing gradients of the other regimes are held to)
      peaked    default x att_k, att_k the first power of two at which >= 30 % of the support rows with two or more entries have their
                largest alpha >= 1 - 1e-6 (asserted here)
      mixed     a1 = -a2 on an x with repeated columns, every operand a small dyadic rational: the scores are EXACT in any order of
                summation, exactly 0 between nodes that share a column (the diagonal included) and of both signs elsewhere
  cell_<setting>_{params, grads, H}   the edge-gated GGCRNNCell of the dir17 case (G 3, F 7, Kin 3, Kst 2, T 3, B 2, bias), loss
      sum(H * cell_R), the gradients of every parameter, of h0 ('h0') and of X ('X'), for the (input, forget) mixers
      zero_zero, peaked_peaked, zero_peaked, default_default (peaked = default x cell_k, chosen as above over every step of both gates)
  cell_peaked_offset   (a1 + a2) . W b of the peaked (input, forget) attention: the score offset the cell's bias puts on every entry
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                   # noqa: E402  (imports the reference, float64 default)
from make_golden import gml, sd_np, grads_np, save    # noqa: E402

ONE_HOT, SHARE = 1.0 - 1e-6, 0.30


def gso_dir17():
    """tests/test_small_edge_train.py::gso_dir17, restated (the CPU test holds the stored S to that function's array)."""
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


def scores_and_alpha(x, a, W, S):
    """(scores [B][m][n], alpha [B][m][n], support mask [m][n]) of a one-head, one-edge-feature attention, in numpy."""
    F = W.shape[2]
    N = S.shape[1]
    mask = np.abs(S[0] + np.eye(N)) > 1e-9
    Wx = np.einsum('fg,bgn->bfn', W[0, 0], x)
    s1, s2 = np.einsum('f,bfn->bn', a[0, 0, :F], Wx), np.einsum('f,bfn->bn', a[0, 0, F:], Wx)
    z = s1[:, None, :] + s2[:, :, None]
    e = np.where(z > 0, z, 0.2 * z)
    e = np.where(mask[None], e, -np.inf)
    with np.errstate(invalid='ignore'):
        ex = np.exp(e - np.max(e, axis=2, keepdims=True))
        alpha = np.nan_to_num(ex / ex.sum(axis=2, keepdims=True))
    return z, alpha, mask


def one_hot_share(x, a, W, S):
    _, alpha, mask = scores_and_alpha(x, a, W, S)
    rows = mask.sum(axis=1) >= 2
    return float((alpha.max(axis=2)[:, rows] >= ONE_HOT).mean())


def attention_regimes(S):
    N, G, F, B = S.shape[1], 3, 7, 2
    rng = np.random.default_rng(190)
    torch.manual_seed(190)
    att = gml.GraphAttentional(G, F, 1, 1)
    W0, a0 = att.weight.detach().numpy().copy(), att.mixer.detach().numpy().copy()
    x0 = rng.standard_normal((B, G, N))
    R = rng.standard_normal((B, 1, F, N))
    k = 1.0
    while one_hot_share(x0, k * a0, W0, S) < SHARE:
        k *= 2.0
        assert k <= 2.0 ** 20
    # mixed: dyadic rationals, columns repeated with period 5, a2 = -a1
    xm = np.round(4.0 * rng.standard_normal((B, G, N))) / 4.0
    xm = xm[:, :, np.arange(N) % 5]
    Wm = np.round(8.0 * W0) / 8.0
    am = np.round(8.0 * a0) / 8.0
    am[0, 0, 0] = 0.5
    am[0, 0, F:] = -am[0, 0, :F]
    z, _, mask = scores_and_alpha(xm, am, Wm, S)
    zs = z[:, mask]
    off = mask & ~np.eye(N, dtype=bool)
    assert np.all(z[:, np.eye(N, dtype=bool) & mask] == 0) and (z[:, off] == 0).sum() >= 4
    assert (zs > 0).sum() >= 10 and (zs < 0).sum() >= 10
    assert np.array_equal(z * 256.0, np.round(z * 256.0))                    # every score a multiple of 1/256: exact in any order
    out = {'att_R': R, 'att_k': np.array(k)}
    for name, x, a, W in (('zero', x0, 0.0 * a0, W0), ('default', x0, a0, W0), ('peaked', x0, k * a0, W0), ('mixed', xm, am, Wm)):
        xt, at, Wt = (torch.tensor(v, requires_grad=True) for v in (x, a, W))
        y = gml.graphAttention(xt, at, Wt, torch.tensor(S))
        (y * torch.tensor(R)).sum().backward()
        out['att_' + name] = dict(x=x, a=a, W=W, y=y.detach().numpy(), grad_x=xt.grad.numpy().copy(), grad_a=at.grad.numpy().copy(),
                                  grad_W=Wt.grad.numpy().copy())
        print('attention %-8s one-hot share %.2f  max|grad_a| %.3e' % (name, one_hot_share(x, a, W, S), np.abs(at.grad.numpy()).max()))
    assert one_hot_share(x0, k * a0, W0, S) >= SHARE
    return out


def cell_settings(S):
    """The dir17 case of tests/test_small_edge_train.py (same shapes and the same draw of X, h0 and R)."""
    N, G, F, Kin, Kst, T, B = S.shape[1], 3, 7, 3, 2, 3, 2
    rng = np.random.default_rng(len('dir17') + 7 * T)
    X = rng.standard_normal((B, T, G, N))
    h0 = np.tanh(rng.standard_normal((B, F, N)))
    R = rng.standard_normal((B, T, F, N))
    St = torch.tensor(S)

    def build(ki, kf):
        torch.manual_seed(T + N)
        cell = gml.GGCRNNCell(G, F, Kin, Kst, torch.tanh, False, 'edge', 1, True)
        cell.addGSO(St)
        with torch.no_grad():
            cell.input_attention.mixer.mul_(ki)
            cell.forget_attention.mixer.mul_(kf)
        return cell

    def shares(cell):
        """One-hot share of the input and of the forget attention over every step."""
        H = cell(torch.tensor(X), torch.tensor(h0)).detach()
        p = sd_np(cell)
        out = []
        for att, w, K_, seq in (('input_attention', cell.weight_A, Kin, [X[:, t] for t in range(T)]),
                                ('forget_attention', cell.weight_B, Kst, [h0] + [H[:, t].numpy() for t in range(T - 1)])):
            u = np.concatenate([gml.LSIGF(w.detach(), St, torch.tensor(v), cell.bias.detach()).numpy() for v in seq], axis=0)
            out.append(one_hot_share(u, p[att + '.mixer'], p[att + '.weight'], S))
        return out

    k = 1.0
    while min(shares(build(k, k))) < SHARE or shares(build(0.0, k))[1] < SHARE:
        k *= 2.0
        assert k <= 2.0 ** 20
    out = {'cell_X': X, 'cell_h0': h0, 'cell_R': R, 'cell_k': np.array(k)}
    for name, ki, kf in (('zero_zero', 0.0, 0.0), ('peaked_peaked', k, k), ('zero_peaked', 0.0, k), ('default_default', 1.0, 1.0)):
        cell = build(ki, kf)
        Xt, ht = torch.tensor(X, requires_grad=True), torch.tensor(h0, requires_grad=True)
        H = cell(Xt, ht)
        (H * torch.tensor(R)).sum().backward()
        g = grads_np(cell)
        g['h0'], g['X'] = ht.grad.numpy().copy(), Xt.grad.numpy().copy()
        p = sd_np(cell)
        out['cell_%s_params' % name], out['cell_%s_grads' % name], out['cell_%s_H' % name] = p, g, H.detach().numpy()
        print('cell %-16s one-hot shares (input, forget) %s  max|grad mixer| %.3e %.3e' % (
            name, ['%.2f' % v for v in shares(cell)], np.abs(g['input_attention.mixer']).max(), np.abs(g['forget_attention.mixer']).max()))
        if name == 'peaked_peaked':
            b = p['bias'][:, 0]
            out['cell_peaked_offset'] = np.array([(p[a + '.mixer'][0, 0, :F] + p[a + '.mixer'][0, 0, F:]) @ (p[a + '.weight'][0, 0] @ b)
                                                  for a in ('input_attention', 'forget_attention')])
    return out


if __name__ == '__main__':
    assert mg.TOL > 0
    S = gso_dir17()
    arrays = {'S': S}
    arrays.update(attention_regimes(S))
    arrays.update(cell_settings(S))
    save('g19_attention_regimes', **arrays)
