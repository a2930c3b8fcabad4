"""Cell + output head Linear(F -> 1) shared by all nodes as ONE launch of the wide sequence-resident kernel (csrc/gcrnn_fused_seq32.h VAR
bit 3, gcrnn_fused_forward_wide_head_bf16; ops.fused_cell_forward_wide_head): the regression model's inference forward. The head acts on the
bf16-rounded state with fp32 sums in a fixed order -- pinned (a) tightly to the head applied by hand to the H of the existing wide forward
(code this variant does not touch) and (b) to the fp64 oracle at the bound tests/test_wide.py puts on H itself, times ||w||_1."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from test_wide import _normalized_adjacency, _uniform_cell, bf16_round


# ------------------------------------------------------------------------------------------ CPU: ABI, query, argument checks
def test_wide_head_entry_points_are_declared_and_the_query_answers_without_a_device(monkeypatch):
    from gated_gcrnns_amd import _lib
    for n in ('gcrnn_fused_forward_wide_head_supported', 'gcrnn_fused_forward_wide_head_bf16'):
        assert n in _lib.EXPORTS
    for e in ('GCRNN_SEQ32', 'GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ_KERNEL', 'GCRNN_SEQ32_SPLIT', 'GCRNN_SEQ32P', 'GCRNN_SEQ32_STATE_SCRATCH'):
        monkeypatch.delenv(e, raising=False)
    q = _lib.lib.gcrnn_fused_forward_wide_head_supported
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.1, 1, 1) == 1
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.1, 1, 0) == 1
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.0, 1, 1) == 0          # weighted graph
    assert q(256, 32, 1000, 64, 64, 5, 4000, 0.1, 1, 1) == 0         # LDS
    assert q(256, 32, 1000, 48, 64, 5, 732, 0.1, 1, 1) == 0          # F = 48
    assert q(100, 32, 1000, 64, 64, 5, 732, 0.1, 1, 1) == 0          # a split batch: one launch per step
    monkeypatch.setenv('GCRNN_SEQ32P', '1')
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.1, 1, 1) == 0
    monkeypatch.delenv('GCRNN_SEQ32P')
    monkeypatch.setenv('GCRNN_SEQ32_STATE_SCRATCH', '0')
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.1, 1, 1) == 0
    monkeypatch.delenv('GCRNN_SEQ32_STATE_SCRATCH')
    assert q(256, 32, 1000, 64, 64, 5, 732, 0.1, 1, 1) == 1


def _entry_args(scratch, scratch_bytes, ptr, head_w, Y, B=256, T=4, N=1000, F=64, G=64, K=5, entries=732):
    return (ptr, ptr, scratch, scratch_bytes, ptr, None, None, None, ptr, ptr, ptr, entries, B, T, N, F, G, K, head_w, None, Y, None, None, None, None)


def test_wide_head_entry_point_validates_before_any_launch(monkeypatch):
    """CPU: every argument check sits in front of the first launch (the pointers are never dereferenced on the host)."""
    from gated_gcrnns_amd import _lib
    for e in ('GCRNN_SEQ32', 'GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ_KERNEL', 'GCRNN_SEQ32_SPLIT'):
        monkeypatch.delenv(e, raising=False)
    lib = _lib.lib
    need = lib.gcrnn_fused_forward_wide_scratch_bytes(256, 64, 0)
    assert need == 256 * 65536
    buf = (C.c_char * 96)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)
    f = lib.gcrnn_fused_forward_wide_head_bf16
    assert f(*_entry_args(ptr, need, ptr, ptr, None)) == 3           # GCRNN_ERR_NULL_POINTER: no Y
    assert f(*_entry_args(ptr, need, ptr, None, ptr)) == 3           # ... no head weights
    assert f(*_entry_args(ptr, need - 1, ptr, ptr, ptr)) == 2        # GCRNN_ERR_BAD_SHAPE: scratch too small
    assert f(*_entry_args(None, need, ptr, ptr, ptr)) == 2           # bytes promised, no pointer
    assert f(*_entry_args(C.c_void_p(ptr.value + 4), need, ptr, ptr, ptr)) == 2      # misaligned scratch
    assert f(*_entry_args(ptr, need, ptr, ptr, ptr, B=4096, T=1024, N=1000)) == 2      # B*T*N past the 32-bit offsets (nothing else is)
    assert f(*_entry_args(ptr, need, ptr, ptr, ptr, B=100)) == 4     # GCRNN_ERR_UNSUPPORTED: a split batch


# ------------------------------------------------------------------------------------------ GPU: parity
# (N, F, G, K, B, T, kind): kind 'u' un-gated, 'tg' time-gated, 'r1' rank-1 (the normalised adjacency of the same kind of graph),
# 'nopk' caller-packed input (GCRNN_NO_INLINE_PACK=1)
SHAPES = {
    'base': (1000, 64, 64, 5, 5, 4, 'u'),
    't32': (1000, 64, 64, 5, 2, 32, 'u'),                # register hand-over 31 times
    'one_chunk': (400, 32, 32, 3, 7, 3, 'u'),            # no scratch
    'g1': (1000, 64, 1, 3, 3, 3, 'u'),                   # padded input
    'b260': (1008, 64, 64, 5, 260, 3, 'u'),              # more sequences than workgroups (scratch reused), partial last tile
    'small': (200, 32, 32, 5, 4, 6, 'u'),
    'gated': (1000, 64, 64, 5, 3, 4, 'tg'),
    'rank1': (400, 64, 64, 3, 3, 3, 'r1'),
    'nopk': (1000, 64, 64, 5, 5, 4, 'nopk'),
}
_REF = {}


def _case(name, dev):
    """Problem, cell on the device, head, and the two references -- computed once per shape, shared by the tests, never written to."""
    if name in _REF:
        return _REF[name]
    import gated_gcrnns_amd.Utils.graphML as gml
    N, F, G, K, B, T, kind = SHAPES[name]
    if kind == 'r1':
        S, rng = _normalized_adjacency(N, 71, 'sym')
        torch.manual_seed(71)
        cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, False, None, 1, True)
        cell.addGSO(torch.tensor(S))
        cell = cell.to(torch.bfloat16)
    else:
        cell, rng, S = _uniform_cell(N, G, F, K, 71, time_gating=(kind == 'tg'))
    X = bf16_round(rng.standard_normal((B, T, G, N)))
    h0 = bf16_round(0.3 * rng.standard_normal((B, F, N)))
    w = rng.uniform(-1.0, 1.0, F) / np.sqrt(F)
    w = torch.tensor(w, dtype=torch.float32).double().numpy()      # the fp32 values the kernel reads
    hb = float(np.float32(0.37))
    params = {k: v.detach().double().numpy() for k, v in cell.state_dict().items()}
    nb = min(B, 3)
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X[:nb], h0[:nb], kind == 'tg', None)
    yref = np.einsum('f,btfn->btn', w, Href) + hb
    cell = cell.to(dev)
    c = dict(N=N, F=F, G=G, K=K, B=B, T=T, kind=kind, cell=cell, yref=yref, nb=nb, w=w,
             Xd=torch.tensor(X, dtype=torch.bfloat16, device=dev), hd=torch.tensor(h0, dtype=torch.bfloat16, device=dev),
             head=(torch.tensor(w, dtype=torch.float32, device=dev).view(1, F), torch.tensor([hb], dtype=torch.float32, device=dev)))
    _REF[name] = c
    return c


def _env(monkeypatch, kind):
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    monkeypatch.setenv('GCRNN_SEQ32P', '0')
    monkeypatch.delenv('GCRNN_NO_WIDE_HEAD', raising=False)
    if kind == 'nopk':
        monkeypatch.setenv('GCRNN_NO_INLINE_PACK', '1')


def _direct(c, out=None, sl=None):
    from gated_gcrnns_amd import ops
    cell = c['cell']
    Xd, hd = (c['Xd'], c['hd']) if sl is None else (c['Xd'][sl].contiguous(), c['hd'][sl].contiguous())
    gates = cell._fused_gates() if c['kind'] == 'tg' else None
    with torch.no_grad():
        return ops.fused_cell_forward_wide_head(Xd, hd, ops.fused_pad_taps(cell.weight_A), cell.weight_B, cell.bias, cell.graph, c['head'],
                                                gates=gates, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_wide_head_matches_the_head_of_the_wide_forward_and_the_oracle(name, monkeypatch):
    from gated_gcrnns_amd import _lib, ops
    dev = torch.device('cuda:0')
    c = _case(name, dev)
    N, F, G, K, B, T, kind = (c[k] for k in ('N', 'F', 'G', 'K', 'B', 'T', 'kind'))
    _env(monkeypatch, kind)
    assert ops.fused_wide_head_supported(c['cell'].graph, B, T, N, F, ops.fused_padded_inputs(F, G), K, kind == 'tg')
    launches = []
    orig = _lib.lib.gcrnn_fused_forward_wide_head_bf16
    monkeypatch.setattr(_lib.lib, 'gcrnn_fused_forward_wide_head_bf16', lambda *a: (launches.append(1), orig(*a))[1], raising=False)
    y = _direct(c)
    assert len(launches) == 1
    assert tuple(y.shape) == (B, T, 1, N) and y.dtype == torch.float32
    y = y[:, :, 0]
    # tight: the head by hand (fp64) on the H of the existing wide forward of the same build
    with torch.no_grad():
        H = c['cell'](c['Xd'], c['hd'])
    w64 = torch.tensor(c['w'], dtype=torch.float64, device=dev)
    want = torch.einsum('f,btfn->btn', w64, H.double()) + c['head'][1].double()
    tight = float((y.double() - want).abs().max())
    wmax = float(want.abs().max())
    # oracle: the bound tests/test_wide.py puts on H (5e-3; 6e-2 at G = 1) times ||w||_1
    tolH = 6.0e-2 if G == 1 else 5.0e-3
    w1 = float(np.abs(c['w']).sum())
    eo = float(np.abs(y[:c['nb']].double().cpu().numpy() - c['yref']).max())
    print('%s: |y - head(H_wide)| max %.3e (bound %.3e), |y - head(H_oracle)| max %.3e (bound %.3e)' % (name, tight, 1e-5 * max(1.0, wmax), eo, w1 * tolH))
    assert wmax > 0.1
    assert tight <= 1e-5 * max(1.0, wmax), tight
    assert eo <= w1 * tolH, (eo, w1 * tolH)
    # out=: a view into a larger buffer keeps every sentinel outside, none inside
    sent = -12345.0
    buf = torch.full((B * T * N + 2 * 64,), sent, dtype=torch.float32, device=dev)
    yo = _direct(c, out=buf[64:64 + B * T * N].view(B, T, N))
    assert bool((buf[:64] == sent).all()) and bool((buf[64 + B * T * N:] == sent).all())
    assert not bool((buf[64:64 + B * T * N] == sent).any())
    # determinism: two calls, equal bits (and the out= call is the same launch)
    assert torch.equal(yo[:, :, 0], y) and yo.data_ptr() == buf[64:].data_ptr()
    if name == 'b260':
        # batch independence: the first three sequences alone (a batch of 3 walks other workgroups and scratch blocks)
        y3 = _direct(c, sl=slice(0, 3))
        assert torch.equal(y3[:, :, 0], y[:3])


@pytest.mark.gpu
def test_wide_head_raises_where_the_form_does_not_apply(monkeypatch):
    """A weighted graph has no bf16-image plan: the explicit entry raises, the dispatch keeps the step kernel."""
    import gated_gcrnns_amd.Utils.graphML as gml
    from gated_gcrnns_amd import ops
    dev = torch.device('cuda:0')
    N, F, K, B, T = 400, 32, 3, 3, 3
    S, rng = _normalized_adjacency(N, 5, 'sym')
    S = S * rng.uniform(0.5, 1.0, S.shape)
    torch.manual_seed(5)
    cell = gml.GGCRNNCell(F, F, K, K, torch.tanh, False, None, 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.to(torch.bfloat16).to(dev)
    _env(monkeypatch, 'u')
    assert not ops.fused_wide_head_supported(cell.graph, B, T, N, F, F, K)
    Xd = torch.randn(B, T, F, N, device=dev).to(torch.bfloat16)
    hd = torch.zeros(B, F, N, device=dev, dtype=torch.bfloat16)
    head = (torch.randn(1, F, device=dev), None)
    with torch.no_grad(), pytest.raises(RuntimeError):
        ops.fused_cell_forward_wide_head(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head)
    with torch.no_grad():
        y = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head=head)
    assert tuple(y.shape) == (B, T, 1, N)


# ------------------------------------------------------------------------------------------ GPU: model level
def _model(tg, dev, N=1000, F=64, G=64, K=5, seed=51):
    import gated_gcrnns_amd.Modules.architectures as archit
    rng = np.random.default_rng(seed)
    W = (rng.random((N, N)) < 10.0 / N).astype(np.float64)
    W = np.triu(W, 1); W = W + W.T
    S = W / np.max(np.abs(np.linalg.eigvalsh(W)))
    torch.manual_seed(17)
    m = archit.GatedGCRNNforRegression(G, F, K, K, torch.tanh, torch.nn.ReLU, [1], S, True, time_gating=tg, spatial_gating=None,
                                       mlpType='multipMlp').to(dev).float()
    return m, rng


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
def test_regression_model_inference_runs_the_wide_head(tg, monkeypatch):
    from gated_gcrnns_amd import _lib, ops
    dev = torch.device('cuda:0')
    N, F, G, K, B, T = 1000, 64, 64, 5, 5, 4
    m, rng = _model(tg, dev)
    X = torch.tensor(rng.standard_normal((B, T, G, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    h0 = torch.tensor(0.3 * rng.standard_normal((B, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    _env(monkeypatch, 'u')
    launches = []
    orig = _lib.lib.gcrnn_fused_forward_wide_head_bf16
    monkeypatch.setattr(_lib.lib, 'gcrnn_fused_forward_wide_head_bf16', lambda *a: (launches.append(1), orig(*a))[1], raising=False)
    cell, lin = m.stateGCRNN, m.outputNN[0]
    with torch.no_grad():
        y = m(X, h0)
        assert len(launches) == 1
        yd = ops.fused_cell_forward_wide_head(X, h0, ops.fused_pad_taps(cell.weight_A), cell.weight_B, cell.bias, cell.graph, (lin.weight, lin.bias),
                                              gates=cell._fused_gates() if tg else None)
        monkeypatch.setenv('GCRNN_NO_WIDE_HEAD', '1')                # the step kernel's head (EPI == 6)
        ys = m(X, h0)
        assert len(launches) == 2
        H = cell(X, h0)
        want = torch.einsum('of,btfn->bton', lin.weight.double(), H.double()) + lin.bias.double().view(1, 1, -1, 1)
    assert tuple(y.shape) == (B, T, 1, N) and y.dtype == X.dtype
    assert torch.equal(y, yd.to(X.dtype))
    d = float((y.double() - ys.double()).abs().max())
    print('wide head vs step-kernel head (bf16 outputs): max %.3e, bound %.3e' % (d, float(want.abs().max()) / 128))
    assert d <= 1.0 / 128 * float(want.abs().max()), d


# ------------------------------------------------------------------------------------------ GPU: capture
@pytest.mark.gpu
def test_wide_head_model_forward_is_capturable(monkeypatch):
    """One torch.cuda.graph capture of the model forward on a side stream: replays give the eager bits, and read the live head weight."""
    dev = torch.device('cuda:0')
    N, F, G, K, B, T = 400, 32, 32, 3, 4, 3
    m, rng = _model(False, dev, N=N, F=F, G=G, K=K, seed=53)
    X = torch.tensor(rng.standard_normal((B, T, G, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    h0 = torch.tensor(0.3 * rng.standard_normal((B, F, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    _env(monkeypatch, 'u')
    from gated_gcrnns_amd import ops
    assert ops.fused_wide_head_supported(m.stateGCRNN.graph, B, T, N, F, G, K)
    with torch.no_grad():
        ye = m(X, h0).clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            m(X, h0)                                                 # warm-up on the capture stream
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                yg = m(X, h0)
        torch.cuda.current_stream(dev).wait_stream(side)
        g.replay(); torch.cuda.synchronize()
        y1 = yg.clone()
        g.replay(); torch.cuda.synchronize()
        y2 = yg.clone()
        assert torch.equal(ye, y1) and torch.equal(ye, y2)
        m.outputNN[0].weight.data.mul_(-2.0)
        g.replay(); torch.cuda.synchronize()
        y3 = yg.clone()
        assert torch.equal(m(X, h0), y3) and not torch.equal(y3, ye)
