"""Plain-torch fp64 restatement of the numpy oracle (TEST INFRASTRUCTURE, NOT PRODUCT).

The same equations as oracle/gcrnn_oracle.py, written with torch's own dense ops on a dense GSO so
that autograd supplies reference gradients. It calls nothing of this library: on a ROCm device it runs on torch's dense
kernels, which are independent of the HIP kernels under test. It runs on whatever device and in whatever dtype its inputs
have; the tests hand it fp64.

Who may import it: tests/ and tools/ only, as the checker. The product (gated_gcrnns_amd/) never imports it.

Conventions are the oracle's (and the reference's):
  * h (filter taps)  : F x E x K x G
  * S (GSO)          : E x N x N dense tensor, row-vector shift x @ S
  * x                : B x G x N ; sequences X : B x T x G x N
  * parameters       : a dict keyed by the module's state_dict keys (cell.state_dict() can be passed as it is).
Quirks kept as the oracle keeps them: the one bias is added by both filters of a step, every gate reads (x_t, h0), and
the output gate (GFL_out / MLP_out) is built but never used.
"""
import torch

ZERO_TOLERANCE = 1e-9      # graphML.py:42
INFINITE_NUMBER = 1e12     # graphML.py:43

ACTS = {None: lambda t: t, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


def lsigf(h, S, x, b=None):
    """y[b,f,n] = sum_e sum_k sum_g h[f,e,k,g] (x S_e^k)[b,g,n] + b[f]   (oracle.lsigf)."""
    F, E, K, G = h.shape
    assert S.shape[0] == E and S.shape[1] == S.shape[2]
    assert x.shape[1] == G and x.shape[2] == S.shape[1]
    y = None
    for e in range(E):
        z = x
        for k in range(K):
            if k > 0:
                z = z @ S[e]
            t = torch.einsum('fg,bgn->bfn', h[:, e, k, :], z)
            y = t if y is None else y + t
    if b is not None:
        y = y + b.reshape(1, F, -1)
    return y


def graph_filter(weight, bias, S, x):
    """GraphFilter.forward with the Nin < N zero pad and trim (oracle.graph_filter)."""
    N, Nin = S.shape[1], x.shape[2]
    if Nin < N:
        x = torch.cat([x, x.new_zeros((x.shape[0], x.shape[1], N - Nin))], dim=2)
    u = lsigf(weight, S, x, bias)
    return u[:, :, :Nin] if Nin < N else u


def graph_filter_layer(weight, bias, S, x, act=None):
    """act(LSIGF(weight, S, x, bias)) for x [items][F_in][N] (ops.graph_filter_layer's contract); act in ACTS."""
    return ACTS[act](lsigf(weight, S, x, bias))


def graph_attention(x, a, W, S, negative_slope=0.2):
    """Dense GAT used as the edge gate (oracle.graph_attention). x: B x G x N, a: K x E x 2F, W: K x E x F x G -> B x K x F x N."""
    N = x.shape[2]
    F = W.shape[2]
    E = a.shape[1]
    assert a.shape[2] == 2 * F
    S = S + torch.eye(N, dtype=S.dtype, device=S.device).reshape(1, N, N)
    Wx = torch.einsum('kefg,bgn->bkefn', W, x)
    a1Wx = torch.einsum('kef,bkefn->bken', a[:, :, :F], Wx)
    a2Wx = torch.einsum('kef,bkefn->bken', a[:, :, F:], Wx)
    aWx = a1Wx[:, :, :, None, :] + a2Wx[:, :, :, :, None]          # [m, n] = a1.Wx_n + a2.Wx_m
    eij = torch.where(aWx > 0, aWx, negative_slope * aWx)          # slope at exactly 0: the negative one (nn.functional.leaky_relu)
    mask = (S.abs().sum(dim=0) > ZERO_TOLERANCE).to(x.dtype)
    logits = eij * mask - (1.0 - mask) * INFINITE_NUMBER
    aij = torch.softmax(logits, dim=4) * mask
    y = torch.einsum('bkefm,bkemn->bkefn', Wx, S.reshape(1, 1, E, N, N) * aij)
    return y.sum(dim=2)


def graph_attentional(mixer, weight, S, x):
    """GraphAttentional.forward with concatenate=True and ReLU (oracle.graph_attentional): B x (K F) x N."""
    y = torch.relu(graph_attention(x, mixer, weight, S))
    B, K, F, N = y.shape
    return y.reshape(B, K * F, N)


def _sub(params, prefix):
    n = len(prefix)
    return {k[n:]: v for k, v in params.items() if k.startswith(prefix)}


def _plain_step(p, S, x, h, sigma):
    b = p.get('bias')
    return sigma(lsigf(p['weight_A'], S, x, b) + lsigf(p['weight_B'], S, h, b))


def ggcrnn_cell(params, S, X, h0, time_gating=False, spatial_gating=None, sigma=torch.tanh):
    """GGCRNNCell.forward (oracle.ggcrnn_cell). X: B x T x G x N, h0: B x F x N -> H: B x T x F x N."""
    B, T = X.shape[0], X.shape[1]
    assert h0.shape[0] == B
    A, Bw, b = params['weight_A'], params['weight_B'], params.get('bias')
    F = A.shape[0]
    N = S.shape[1]
    one = X.new_ones((B, 1, 1))
    H = []
    h = h0
    for t in range(T):
        x = X[:, t]
        gi = gf = one
        if time_gating:
            ci = _plain_step(_sub(params, 'GFL_in.'), S, x, h0, sigma).reshape(B, F * N)
            gi = torch.sigmoid(ci @ params['MLP_in.0.weight'].t() + params.get('MLP_in.0.bias', 0.0)).reshape(B, 1, 1)
            cf = _plain_step(_sub(params, 'GFL_forget.'), S, x, h0, sigma).reshape(B, F * N)
            gf = torch.sigmoid(cf @ params['MLP_forget.0.weight'].t() + params.get('MLP_forget.0.bias', 0.0)).reshape(B, 1, 1)
        ya = lsigf(A, S, x, b)
        yb = lsigf(Bw, S, h, b)
        if spatial_gating == 'node':
            di = _plain_step(_sub(params, 'GRNN_node_in.'), S, x, h0, sigma)
            ni = torch.sigmoid(graph_filter(params['GFL_node_in.0.weight'], params.get('GFL_node_in.0.bias'), S, di))
            df = _plain_step(_sub(params, 'GRNN_node_forget.'), S, x, h0, sigma)
            nf = torch.sigmoid(graph_filter(params['GFL_node_forget.0.weight'], params.get('GFL_node_forget.0.bias'), S, df))
            h = sigma(gi * (ni * ya) + gf * (nf * yb))
        elif spatial_gating == 'edge':
            ya = graph_attentional(params['input_attention.mixer'], params['input_attention.weight'], S, ya)
            yb = graph_attentional(params['forget_attention.mixer'], params['forget_attention.weight'], S, yb)
            h = sigma(gi * ya + gf * yb)
        else:
            h = sigma(gi * ya + gf * yb)
        H.append(h)
    return torch.stack(H, dim=1)


def selection_gnn(params, S, x, act='relu'):
    """SelectionGNN with NoPool (reference architectures.py:10-177): graph-filter layers GFL.<3l> each followed by `act`, then the
    MLP (Linear layers MLP.<i>, `act` between them) on the flattened [B][F N] signal. x: B x F_0 x N."""
    layers = sorted({int(k.split('.')[1]) for k in params if k.startswith('GFL.')})
    y = x
    for l in layers:
        y = graph_filter_layer(params['GFL.%d.weight' % l], params.get('GFL.%d.bias' % l), S, y, act)
    y = y.reshape(y.shape[0], -1)
    mlp = sorted({int(k.split('.')[1]) for k in params if k.startswith('MLP.')})
    for j, i in enumerate(mlp):
        if j > 0:
            y = ACTS[act](y)
        y = y @ params['MLP.%d.weight' % i].t()
        if 'MLP.%d.bias' % i in params:
            y = y + params['MLP.%d.bias' % i]
    return y
