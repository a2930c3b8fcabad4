"""Self-start of the wide inference forward (csrc/gcrnn_fused_seq32.h, Seq32Args::self_start; C entry gcrnn_fused_forward_wide_user_bf16, or
GCRNN_WIDE_SELF_START in gcrnn_fused_forward_wide_scratch_bf16's flags, which is what ops.fused_cell_forward issues): the persistent launch
reads h0 and x_0 from the USER-layout tensors itself (whole 32-feature k-steps staged through the idle hop-image planes) and lays out x_1
during step 0, so no gcrnn_pack_seq_major / gcrnn_pack_seq_major_steps launch runs in front of it. The change moves bytes and performs no
arithmetic: H is BIT-identical to the path with the caller's layout launches (GCRNN_SEQ32_SELF_START=0, read by the library at every call),
which stays pinned to the fp64 oracle by tests/test_wide.py and tests/test_state_scratch.py.
T <= 2: the self-start form takes them too (it needs no caller-packed x_1); pinned below by the launch counts of the T = 1, 2 cases.
The form launches one workgroup per SEQUENCE (every sequence gets the start-up phase; beyond one per CU the later ones start as CUs free up).
The output-head launch has the same form (gcrnn_fused_forward_wide_head_user_bf16), opt-in through
ops.fused_cell_forward_wide_head(self_start=True): tests/test_wide_head.py pins the default dispatch of fused_cell_forward(head=...) to ONE
call of gcrnn_fused_forward_wide_head_bf16, whose argument list has no room for the switch."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from test_wide import _normalized_adjacency, _uniform_cell, bf16_round

_PACKS = ('gcrnn_pack_seq_major', 'gcrnn_pack_seq_major_steps')
_FWD = 'gcrnn_fused_forward_wide_scratch_bf16'


class _Calls(object):
    """Counts the layout launches and the forward entry point; of the latter also how many calls carried GCRNN_WIDE_SELF_START (argument 19,
    huser_last_only). The ctypes functions are looked up on the library object at every call."""

    def __init__(self, monkeypatch):
        from gated_gcrnns_amd import _lib
        self.n = {'packs': 0, 'fwd': 0, 'self': 0}
        for name in _PACKS + (_FWD,):
            orig = getattr(_lib.lib, name)

            def wrapped(*a, _orig=orig, _name=name):
                if _name == _FWD:
                    self.n['fwd'] += 1
                    self.n['self'] += 1 if (int(a[19]) & 2) else 0
                else:
                    self.n['packs'] += 1
                return _orig(*a)
            monkeypatch.setattr(_lib.lib, name, wrapped, raising=False)


def _both(cell, Xd, hd, monkeypatch, **kw):
    """H with the self-start (one forward call carrying the flag, no layout launch) and with the switch at 0 (the old counts: one pack of
    h0, one of the leading steps of X, one forward call without the flag)."""
    calls = _Calls(monkeypatch)
    s, p = 1, 0
    with torch.no_grad():
        monkeypatch.delenv('GCRNN_SEQ32_SELF_START', raising=False)
        H = cell(Xd, hd, **kw)
        torch.cuda.synchronize()
        assert calls.n == {'packs': p, 'fwd': 1, 'self': s}, calls.n
        monkeypatch.setenv('GCRNN_SEQ32_SELF_START', '0')
        H0 = cell(Xd, hd, **kw)
        torch.cuda.synchronize()
        assert calls.n == {'packs': p + 2, 'fwd': 2, 'self': s}, calls.n
        monkeypatch.delenv('GCRNN_SEQ32_SELF_START')
    return H, H0


def _problem(N, F, G, K, B, T, seed=89, dev=None, hzero=False):
    cell, rng, S = _uniform_cell(N, G, F, K, seed)
    X = bf16_round(rng.standard_normal((B, T, G, N)))
    h0 = bf16_round(0.3 * rng.standard_normal((B, F, N)))          # non-zero h0: the start-up reads it from the caller's tensor
    if hzero:
        h0 = np.zeros_like(h0)
    Xd = torch.tensor(X, dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(h0, dtype=torch.bfloat16, device=dev)
    return cell, S, X, h0, Xd, hd


# (N, F, G, K, B, T, last_only, h0 zero): the smallest shapes at which each branch of the start-up can go wrong --
#  n1000: the last staged columns are partial (1000 = 7 * 128 + 104); b260: more sequences than CUs -- four sequences start on CUs that have
#  already run one, and keep their state in slot 0 of the work buffer (the scratch is sized by one workgroup per CU);
#  n400 / n200: whole column ranges never fetched, F = 32 (one chunk: nothing reloaded); g32: XS = 1; k3 / k2: RPH = 2 / 4, several x_1
#  rounds at the start-up; T = 1, 2, 3; the last state only; an all-zero h0.
CASES = {
    'n1000': (1000, 64, 64, 5, 4, 5, False, False),
    'b260': (1008, 64, 64, 5, 260, 4, False, False),
    'n400_f32_k3': (400, 32, 32, 3, 4, 5, False, False),
    'n200_f32': (200, 32, 32, 5, 4, 6, False, False),
    'g32_k4': (1000, 64, 32, 4, 4, 5, False, False),
    'k3': (1000, 64, 64, 3, 4, 5, False, False),
    'k2': (1000, 64, 64, 2, 4, 5, False, False),
    't1': (1000, 64, 64, 5, 5, 1, False, False),
    't2': (1000, 64, 64, 5, 5, 2, False, False),
    't3': (1000, 64, 64, 5, 5, 3, False, False),
    'last_only': (1000, 64, 64, 5, 4, 5, True, False),
    'h0_zero': (1000, 64, 64, 5, 4, 5, False, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_self_start_is_bit_identical_to_the_caller_packed_path(case, monkeypatch):
    N, F, G, K, B, T, last_only, hz = CASES[case]
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev, hzero=hz)
    cell = cell.to(dev)
    if B < 129:
        monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')              # (small batches: onto the persistent wide kernel, as tests/test_wide.py does)
    H, H0 = _both(cell, Xd, hd, monkeypatch, **({'last_only': True} if last_only else {}))
    assert tuple(H.shape) == (B, 1 if last_only else T, F, N)
    assert torch.equal(H, H0), float((H.float() - H0.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1                     # (not two all-zero tensors)


@pytest.mark.gpu
def test_self_start_on_a_rank1_weighted_graph_is_bit_identical(monkeypatch):
    import gated_gcrnns_amd.Utils.graphML as gml
    dev = torch.device('cuda:0')
    N, F, K, B, T = 1000, 64, 5, 4, 5
    S, rng = _normalized_adjacency(N, 47, 'sym')
    torch.manual_seed(47)
    cell = gml.GGCRNNCell(F, F, K, K, torch.tanh, False, None, 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.to(torch.bfloat16).to(dev)
    Xd = torch.tensor(bf16_round(rng.standard_normal((B, T, F, N))), dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(bf16_round(0.3 * rng.standard_normal((B, F, N))), dtype=torch.bfloat16, device=dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    H, H0 = _both(cell, Xd, hd, monkeypatch)
    assert torch.equal(H, H0), float((H.float() - H0.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize('B', [4, 260])
def test_self_start_output_head_is_bit_identical(B, monkeypatch):
    """The output-head launch (VAR 13): y of the self-start form against y of the caller-packed head launch, bit for bit; the new entry point
    ran once and no layout launch did. B = 260: more sequences than CUs."""
    from gated_gcrnns_amd import _lib, ops
    N, F, G, K, T = 1000, 64, 64, 5, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, seed=91, dev=dev)
    cell = cell.to(dev)
    if B < 129:
        monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    torch.manual_seed(3)
    head = (torch.randn(1, F, device=dev), torch.randn(1, device=dev))
    n = {'packs': 0, 'user': 0, 'old': 0}
    for key, names in (('packs', _PACKS), ('user', ('gcrnn_fused_forward_wide_head_user_bf16',)), ('old', ('gcrnn_fused_forward_wide_head_bf16',))):
        for name in names:
            orig = getattr(_lib.lib, name)

            def wrapped(*a, _orig=orig, _key=key):
                n[_key] += 1
                return _orig(*a)
            monkeypatch.setattr(_lib.lib, name, wrapped, raising=False)
    with torch.no_grad():
        y = ops.fused_cell_forward_wide_head(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head, self_start=True)
        torch.cuda.synchronize()
        assert n == {'packs': 0, 'user': 1, 'old': 0}, n
        y0 = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, head=head)
        torch.cuda.synchronize()
        assert n == {'packs': 2, 'user': 1, 'old': 1}, n
    assert tuple(y.shape) == (B, T, 1, N) and y.dtype == torch.float32
    assert torch.equal(y, y0), float((y - y0).abs().max())
    assert float(y.abs().max()) > 0.1


@pytest.mark.gpu
def test_self_start_c_entry_point_is_the_same_launch(monkeypatch):
    """gcrnn_fused_forward_wide_user_bf16 called directly: the cell's H; a work buffer one byte short returns GCRNN_ERR_BAD_SHAPE and H
    keeps the caller's bytes."""
    from gated_gcrnns_amd import _lib, ops
    N, F, G, K, B, T = 1000, 64, 64, 5, 4, 3
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    plan = ops.fused_wide_user_plan(cell.graph, Xd, hd, F, G, K)
    assert plan is not None
    st = ops._stream()
    wpw, b32 = ops._fused_pack_weights_wide_bias(cell.weight_A.detach(), cell.weight_B.detach(), cell.bias, plan['uniform_w'], st)
    assert torch.equal(b32, cell.bias.detach().float().view(-1))
    assert torch.equal(wpw, ops._fused_pack_weights_wide(cell.weight_A.detach(), cell.weight_B.detach(), plan['uniform_w'], st))
    need = int(_lib.lib.gcrnn_fused_forward_wide_user_bytes(B, T, G))
    assert need == T * B * 1024 * G * 2
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    scr = ops.fused_state_scratch(plan, B, F, dev)
    H = torch.full((B, T, F, N), 7.0, dtype=torch.bfloat16, device=dev)
    p = ops._p

    def call(nbytes):
        return _lib.lib.gcrnn_fused_forward_wide_user_bf16(p(work), nbytes, p(hd), p(scr), int(scr.numel()), p(wpw), p(b32), p(plan['tile_slots']),
                                                           p(plan['tile_off']), p(plan['ell_col4']), plan['entries'], B, T, N, F, G, K, p(H), 0,
                                                           p(Xd), None, None, st)
    assert call(need - 1) == 2
    torch.cuda.synchronize()
    assert bool((H == 7.0).all())
    assert call(need) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(H, cell(Xd, hd))


@pytest.mark.gpu
def test_self_start_matches_oracle_at_the_bench_shape(monkeypatch):
    """The self-start launch against the fp64 oracle on the bf16-rounded operands at the bench shape (B = 256: every workgroup of the chip
    runs), tolerances of tests/test_wide.py for this kernel after T = 32 steps: 5e-3 max, 1e-3 mean. The oracle is dense: three sequences."""
    N, F, G, K, B, T = 1000, 64, 64, 5, 256, 32
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, seed=73, dev=dev)
    params = {k: v.detach().double().numpy() for k, v in cell.state_dict().items()}
    pick = [0, 129, 255]
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X[pick], h0[pick])
    cell = cell.to(dev)
    calls = _Calls(monkeypatch)
    with torch.no_grad():
        H = cell(Xd, hd)
    assert calls.n == {'packs': 0, 'fwd': 1, 'self': 1}, calls.n
    err = np.abs(H[pick].double().cpu().numpy() - Href)
    print('self-start vs oracle, T = 32: max %.3e mean %.3e' % (err.max(), err.mean()))
    assert err.max() <= 5.0e-3 and err.mean() <= 1.0e-3, (err.max(), err.mean())


@pytest.mark.gpu
def test_self_start_is_captured_and_replays_read_the_callers_tensors(monkeypatch):
    """A FusedForwardGraph captures the self-start form and replays the eager call's bits; after X AND h0 were overwritten in place a replay
    gives the new inputs' result -- the kernel reads the caller's tensors at replay time, no laid-out copy of them is part of the graph."""
    from gated_gcrnns_amd import ops
    N, F, G, K, B, T = 1000, 64, 64, 5, 256, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    calls = _Calls(monkeypatch)
    with torch.no_grad():
        He = cell(Xd, hd).clone()
        assert calls.n == {'packs': 0, 'fwd': 1, 'self': 1}, calls.n
        runner = ops.FusedForwardGraph(cell, B, T, X=Xd, h0=hd)
        assert calls.n['packs'] == 0 and calls.n['self'] == calls.n['fwd'] >= 2            # (warm-ups and the capture)
        H1 = runner().clone()
        assert torch.equal(He, H1)
        Xd.copy_(torch.randn(B, T, G, N, device=dev).to(torch.bfloat16))
        hd.copy_((0.3 * torch.randn(B, F, N, device=dev)).to(torch.bfloat16))
        H2 = runner().clone()
        assert torch.equal(cell(Xd, hd), H2) and not torch.equal(H2, He)


# ------------------------------------------------------------------------------------------ CPU: the C ABI
def _user_args(ptr, xs_bytes, scratch_bytes, B=256, T=4, N=1000, F=64, G=64, K=5, entries=732):
    return (ptr, xs_bytes, ptr, ptr, scratch_bytes, ptr, None, ptr, ptr, ptr, entries, B, T, N, F, G, K, ptr, 0, ptr, None, None, None)


def test_self_start_entry_point_validates_before_any_launch():
    """No device is needed to be told that a shape is bad or a buffer too small; the pointers are never dereferenced on the host."""
    from gated_gcrnns_amd import _lib
    lib = _lib.lib
    for n in ('gcrnn_fused_forward_wide_user_bytes', 'gcrnn_fused_forward_wide_user_supported', 'gcrnn_fused_forward_wide_user_bf16',
              'gcrnn_fused_forward_wide_head_user_supported', 'gcrnn_fused_forward_wide_head_user_bf16', 'gcrnn_fused_pack_weights_wide_bias'):
        assert n in _lib.EXPORTS
    need = lib.gcrnn_fused_forward_wide_user_bytes(256, 4, 64)
    assert need == 4 * 256 * 1024 * 64 * 2
    assert lib.gcrnn_fused_forward_wide_user_bytes(0, 4, 64) == -1
    sneed = lib.gcrnn_fused_forward_wide_scratch_bytes(256, 64, 0)
    buf = (C.c_char * 96)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)
    f = lib.gcrnn_fused_forward_wide_user_bf16
    assert f(*_user_args(ptr, need, sneed, N=1004)) == 2         # GCRNN_ERR_BAD_SHAPE: N % 8 != 0
    assert f(*_user_args(ptr, need, sneed, F=48)) == 4           # GCRNN_ERR_UNSUPPORTED: F % 32 != 0
    assert f(*_user_args(ptr, need, sneed, G=16)) == 4
    assert f(*_user_args(ptr, need - 1, sneed)) == 2             # the work buffer is too small
    assert f(*_user_args(ptr, need, sneed - 1)) == 2             # the state scratch is too small
    a = list(_user_args(ptr, need, sneed)); a[2] = None          # h0_user
    assert f(*a) == 3                                            # GCRNN_ERR_NULL_POINTER
    a = list(_user_args(ptr, need, sneed)); a[19] = None         # Xuser is required: x_0 is read from it
    assert f(*a) == 3
    a = list(_user_args(ptr, need, sneed)); a[2] = C.c_void_p(ptr.value + 2)      # a misaligned h0_user
    assert f(*a) == 2
    # the same launch through the scratch entry point's flag: same checks
    g = lib.gcrnn_fused_forward_wide_scratch_bf16

    def flagged(N=1000, F=64):
        return (ptr, ptr, ptr, sneed, ptr, None, None, None, ptr, ptr, ptr, 732, 256, 4, N, F, 64, 5, ptr, 2, ptr, None, None, None)
    assert g(*flagged(N=1004)) == 2 and g(*flagged(F=48)) == 4
    a = list(flagged()); a[20] = None
    assert g(*a) == 3
    a = list(flagged(N=1004)); a[19] = 6                         # only 2 and 3 carry the flag: any other non-zero value is "the last state only"
    assert g(*a) == 2 and g(*flagged(N=1004)) == 2               # (N % 8 != 0 is a bad shape of that launch, too: Huser's 16-byte rows)
    a = list(flagged()); a[19] = 6; a[20] = None; a[3] = sneed - 1      # ... where Xuser is optional: the short scratch is what is reported
    assert g(*a) == 2
    a[19] = 2                                                    # with the flag, the missing Xuser comes first
    assert g(*a) == 3
    # the head form: the same checks
    hf = lib.gcrnn_fused_forward_wide_head_user_bf16

    def head_args(xs_bytes, N=1000, F=64):
        return (ptr, xs_bytes, ptr, ptr, sneed, ptr, None, ptr, ptr, ptr, 732, 256, 4, N, F, 64, 5, ptr, None, ptr, ptr, None, None, None)
    assert hf(*head_args(need, N=1004)) == 2 and hf(*head_args(need, F=48)) == 4 and hf(*head_args(need - 1)) == 2
    # the weight + bias pack
    pk = lib.gcrnn_fused_pack_weights_wide_bias
    assert pk(2, ptr, ptr, None, ptr, ptr, 64, 64, 64, 5, 5, 1.0, None) == 3
    assert pk(2, ptr, ptr, ptr, ptr, ptr, 48, 64, 64, 5, 5, 1.0, None) == 2
    assert pk(1, ptr, ptr, ptr, ptr, ptr, 64, 64, 64, 5, 5, 1.0, None) == 1       # GCRNN_ERR_BAD_DTYPE: fp64 taps


def test_self_start_switch_is_read_at_every_call(monkeypatch):
    from gated_gcrnns_amd import _lib
    q = _lib.lib.gcrnn_fused_forward_wide_user_supported
    args = (256, 32, 1000, 64, 64, 5, 732, 0.5, 1)
    for k in ('GCRNN_SEQ32_SELF_START', 'GCRNN_SEQ32_STATE_SCRATCH', 'GCRNN_SEQ32P', 'GCRNN_SEQ32', 'GCRNN_SEQ32_MIN_B', 'GCRNN_SEQ_KERNEL'):
        monkeypatch.delenv(k, raising=False)
    assert q(*args) == 1
    assert q(256, 1, 1000, 64, 64, 5, 732, 0.5, 1) == 1 and q(256, 2, 1000, 64, 64, 5, 732, 0.5, 3) == 1      # T <= 2 and rank-1 graphs too
    monkeypatch.setenv('GCRNN_SEQ32_SELF_START', '0')
    assert q(*args) == 0
    monkeypatch.setenv('GCRNN_SEQ32_SELF_START', '1')
    assert q(*args) == 1
    monkeypatch.setenv('GCRNN_SEQ32_STATE_SCRATCH', '0')          # no state scratch, no self-start (the state-image launches)
    assert q(*args) == 0
    monkeypatch.delenv('GCRNN_SEQ32_STATE_SCRATCH')
    assert q(100, 32, 1000, 64, 64, 5, 732, 0.5, 1) == 0          # a split batch: one launch per step
    assert q(4096, 32, 1000, 64, 64, 5, 732, 0.5, 1) == 1         # more sequences than CUs: one workgroup per sequence
    qh = _lib.lib.gcrnn_fused_forward_wide_head_user_supported
    assert qh(*args) == 1
    monkeypatch.setenv('GCRNN_SEQ32_SELF_START', '0')
    assert qh(*args) == 0
    monkeypatch.delenv('GCRNN_SEQ32_SELF_START')
    assert q(256, 32, 1004, 64, 64, 5, 732, 0.5, 1) == 0 and q(256, 32, 1000, 48, 64, 5, 732, 0.5, 1) == 0
