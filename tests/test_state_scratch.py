"""The wide forward WITHOUT a state image (csrc/gcrnn_fused_seq32.h VAR bit 2, gcrnn_fused_forward_wide_scratch_bf16): in inference through
the user-layout H the launch keeps the state it re-reads (chunks 0 .. F/32-2 of h_t) in a per-workgroup scratch in slot order and stores
nothing else of the sequence-major state. Only WHERE bytes are stored changes, not one arithmetic operation: H is bit-identical to the
path with the state image (GCRNN_SEQ32_STATE_SCRATCH=0, read by the library at every call), which stays pinned to the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from test_wide import _normalized_adjacency, _uniform_cell, bf16_round


class _Calls(object):
    """Counts the launches of the two entry points (the ctypes functions are looked up on the library object at every call)."""

    def __init__(self, monkeypatch):
        from gated_gcrnns_amd import _lib
        self.n = {'scratch': 0, 'image': 0}
        for key, name in (('scratch', 'gcrnn_fused_forward_wide_scratch_bf16'), ('image', 'gcrnn_fused_forward_wide_bf16')):
            orig = getattr(_lib.lib, name)

            def wrapped(*a, _orig=orig, _key=key):
                self.n[_key] += 1
                return _orig(*a)
            monkeypatch.setattr(_lib.lib, name, wrapped, raising=False)


def _both_paths(cell, Xd, hd, monkeypatch, wide=True, **kw):
    """H on the scratch path and on the state-image path, each checked to have been the launch that ran (wide=False: a problem the wide
    kernel does not take at all -- neither entry point runs, with either setting of the switch)."""
    calls = _Calls(monkeypatch)
    w = 1 if wide else 0
    with torch.no_grad():
        monkeypatch.delenv('GCRNN_SEQ32_STATE_SCRATCH', raising=False)
        H = cell(Xd, hd, **kw)
        torch.cuda.synchronize()
        assert calls.n == {'scratch': w, 'image': 0}, calls.n
        monkeypatch.setenv('GCRNN_SEQ32_STATE_SCRATCH', '0')
        H0 = cell(Xd, hd, **kw)
        torch.cuda.synchronize()
        assert calls.n == {'scratch': w, 'image': w}, calls.n
        monkeypatch.delenv('GCRNN_SEQ32_STATE_SCRATCH')
    return H, H0


def _problem(N, F, G, K, B, T, seed=83, tg=False, dev=None):
    cell, rng, S = _uniform_cell(N, G, F, K, seed, time_gating=tg)
    X = bf16_round(rng.standard_normal((B, T, G, N)))
    h0 = bf16_round(0.3 * rng.standard_normal((B, F, N)))          # non-zero h0 in every case: step 0 reads it from the caller's array
    Xd = torch.tensor(X, dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(h0, dtype=torch.bfloat16, device=dev)
    return cell, S, X, h0, Xd, hd


# (N, F, G, K, B, T, last_only): the bench shape at B = 256 and at B = 300 (workgroups that walk two sequences through one scratch block);
# T = 1, 2, 3 (the inline pack starts at T > 2); the last state only; G = 32; F = 32 (one chunk: nothing stored or reloaded); K = 2, 3, 4;
# N = 1024 (every other case is N = 1000). At N = 1024 there is no padding row to aim the plan's padding entries at, so the bf16-image plan
# does not exist and the forward stays on the 16-feature kernels with either setting of the switch (tests/test_wide.py,
# test_wide_kernel_edge_shapes_match_oracle): the case pins that the switch changes nothing there; it cannot reach the new launch.
CASES = {
    'bench_b256': (1000, 64, 64, 5, 256, 32, False),
    'bench_b300': (1000, 64, 64, 5, 300, 32, False),
    't1': (1000, 64, 64, 5, 5, 1, False),
    't2': (1000, 64, 64, 5, 5, 2, False),
    't3': (1000, 64, 64, 5, 5, 3, False),
    'last_only': (1000, 64, 64, 5, 6, 5, True),
    'g32': (1000, 64, 32, 5, 4, 5, False),
    'f32': (1000, 32, 32, 5, 4, 5, False),
    'k2': (1000, 64, 64, 2, 4, 5, False),
    'k3': (1000, 64, 64, 3, 4, 5, False),
    'k4': (1000, 64, 64, 4, 4, 5, False),
    'n1024': (1024, 64, 64, 5, 4, 5, False),
    'n1024_b260': (1024, 64, 64, 3, 260, 4, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_state_scratch_is_bit_identical_to_the_state_image_path(case, monkeypatch):
    N, F, G, K, B, T, last_only = CASES[case]
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    from gated_gcrnns_amd import ops
    if B < 129:
        monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')              # (small batches: onto the persistent wide kernel, as tests/test_wide.py does)
    wide = ops.fused_wide_plan(cell.graph, B, T, N, F, G, K, T > 2) is not None
    assert wide == (N != 1024)
    H, H0 = _both_paths(cell, Xd, hd, monkeypatch, wide=wide, **({'last_only': True} if last_only else {}))
    assert tuple(H.shape) == (B, 1 if last_only else T, F, N)
    assert torch.equal(H, H0), float((H.float() - H0.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1                     # (not two all-zero tensors)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,hz', [(4, 5, False), (260, 4, False), (4, 5, True)])
def test_state_scratch_time_gated_cell_is_bit_identical(B, T, hz, monkeypatch):
    """The time-gated recurrence (GATED, VAR 6: the gate pre-pass has laid out X)."""
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(1000, 64, 64, 5, B, T, tg=True, dev=dev)
    if hz:
        hd = torch.zeros_like(hd)
    cell = cell.to(dev)
    if B < 129:
        monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    H, H0 = _both_paths(cell, Xd, hd, monkeypatch)
    assert torch.equal(H, H0), float((H.float() - H0.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize('kind,tg,K,F', [('sym', False, 5, 64), ('rw', False, 3, 64), ('sym', True, 5, 64), ('sym', False, 4, 32)])
def test_state_scratch_on_rank1_weighted_graphs_is_bit_identical(kind, tg, K, F, monkeypatch):
    """Normalised adjacencies (R1 instantiations), un-gated with and without the inline pack and time-gated."""
    import gated_gcrnns_amd.Utils.graphML as gml
    dev = torch.device('cuda:0')
    N, B, T = 1000, 4, 5
    S, rng = _normalized_adjacency(N, 43, kind)
    torch.manual_seed(43)
    cell = gml.GGCRNNCell(F, F, K, K, torch.tanh, tg, None, 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.to(torch.bfloat16).to(dev)
    Xd = torch.tensor(bf16_round(rng.standard_normal((B, T, F, N))), dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(bf16_round(0.3 * rng.standard_normal((B, F, N))), dtype=torch.bfloat16, device=dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    H, H0 = _both_paths(cell, Xd, hd, monkeypatch)
    assert torch.equal(H, H0), float((H.float() - H0.float()).abs().max())
    if not tg:
        monkeypatch.setenv('GCRNN_NO_INLINE_PACK', '1')           # VAR 6 of the un-gated rank-1 form
        H2, H20 = _both_paths(cell, Xd, hd, monkeypatch)
        assert torch.equal(H2, H20) and torch.equal(H, H2)


@pytest.mark.gpu
def test_state_scratch_without_the_inline_pack_is_bit_identical(monkeypatch):
    """VAR 6 of the un-gated cell (caller-packed X) at a batch whose workgroups walk two sequences."""
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(1000, 64, 64, 5, 300, 6, dev=dev)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_NO_INLINE_PACK', '1')
    H, H0 = _both_paths(cell, Xd, hd, monkeypatch)
    assert torch.equal(H, H0)
    monkeypatch.delenv('GCRNN_NO_INLINE_PACK')
    with torch.no_grad():
        assert torch.equal(H, cell(Xd, hd))


@pytest.mark.gpu
def test_state_scratch_matches_oracle_at_the_bench_shape(monkeypatch):
    """The new launch against the fp64 oracle at the tolerances tests/test_wide.py holds this kernel to after T = 32 steps (5e-3 max,
    1e-3 mean), at the bench shape (B = 256: every workgroup of the chip runs). The oracle is dense: it runs three of the sequences; all
    256 are compared bit for bit with the state-image path by the test above."""
    N, F, G, K, B, T = 1000, 64, 64, 5, 256, 32
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, seed=71, dev=dev)
    params = {k: v.detach().double().numpy() for k, v in cell.state_dict().items()}
    pick = [0, 129, 255]
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X[pick], h0[pick])
    cell = cell.to(dev)
    calls = _Calls(monkeypatch)
    with torch.no_grad():
        H = cell(Xd, hd)
    assert calls.n == {'scratch': 1, 'image': 0}
    err = np.abs(H[pick].double().cpu().numpy() - Href)
    print('state scratch vs oracle, T = 32: max %.3e mean %.3e (step 0: max %.3e)' % (err.max(), err.mean(), err[:, 0].max()))
    assert err[:, 0].max() <= 4.0e-3, err[:, 0].max()
    assert err.max() <= 5.0e-3 and err.mean() <= 1.0e-3, (err.max(), err.mean())


@pytest.mark.gpu
@pytest.mark.parametrize('tg', [False, True])
def test_state_scratch_replays_bit_identically(tg, monkeypatch):
    """A FusedForwardGraph captured on the new path replays the eager call's bits, twice in a row (the scratch is re-used between replays:
    nothing a replay leaves in it is read by the next one), and again after the caller refills X in place."""
    from gated_gcrnns_amd import ops
    N, F, G, K, B, T = 1000, 64, 64, 5, 256, 6
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, tg=tg, dev=dev)
    cell = cell.to(dev)
    calls = _Calls(monkeypatch)
    with torch.no_grad():
        He = cell(Xd, hd).clone()
        assert calls.n == {'scratch': 1, 'image': 0}
        runner = ops.FusedForwardGraph(cell, B, T, X=Xd, h0=hd)
        assert calls.n['image'] == 0 and calls.n['scratch'] >= 2            # (warm-ups and the capture)
        H1 = runner().clone()
        H2 = runner().clone()
        assert torch.equal(He, H1) and torch.equal(He, H2)
        Xd.copy_(torch.randn(B, T, G, N, device=dev).to(torch.bfloat16))
        H3 = runner().clone()
        assert torch.equal(cell(Xd, hd), H3) and not torch.equal(H3, He)


def _entry_args(scratch, scratch_bytes, ptr, B=256, T=4, N=1000, F=64, G=64, K=5, entries=732):
    return (ptr, ptr, scratch, scratch_bytes, ptr, None, None, None, ptr, ptr, ptr, entries, B, T, N, F, G, K, ptr, 0, None, None, None, None)


def test_scratch_entry_point_validates_before_any_launch():
    """CPU: the size query, and the entry point's argument checks -- all of them in front of the first launch (no device is needed to be
    told that the scratch is too small; the pointers are never dereferenced on the host)."""
    from gated_gcrnns_amd import _lib
    lib = _lib.lib
    for n in ('gcrnn_fused_forward_wide_scratch_bytes', 'gcrnn_fused_forward_wide_scratch_bf16'):
        assert n in _lib.EXPORTS
    need = lib.gcrnn_fused_forward_wide_scratch_bytes(256, 64, 0)
    assert need == 256 * 1024 * 32 * 2                           # [workgroups][1024 slots][32] bf16: 16 MB whatever B is beyond the grid
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(300, 64, 0) == need and lib.gcrnn_fused_forward_wide_scratch_bytes(4096, 64, 1) == need
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(200, 64, 0) == 200 * 65536
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(256, 32, 0) == 0          # one chunk: handed over in registers, nothing to keep
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(100, 64, 0) == -1         # split sequences: one launch per step
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(100, 64, 1) == 100 * 65536
    assert lib.gcrnn_fused_forward_wide_scratch_bytes(256, 48, 0) == -1 and lib.gcrnn_fused_forward_wide_scratch_bytes(0, 64, 0) == -1
    buf = (C.c_char * 96)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)              # (16-byte aligned, as the entry point asks of Huser)
    f = lib.gcrnn_fused_forward_wide_scratch_bf16
    assert f(*_entry_args(ptr, need - 1, ptr)) == 2              # GCRNN_ERR_BAD_SHAPE: too small
    assert f(*_entry_args(ptr, 0, ptr)) == 2
    assert f(*_entry_args(None, need, ptr)) == 2                 # bytes promised, no pointer
    a = list(_entry_args(ptr, need, ptr)); a[18] = None          # Huser is required: there is no other output
    assert f(*a) == 3                                            # GCRNN_ERR_NULL_POINTER
    assert f(*_entry_args(ptr, need, ptr, B=100)) == 4           # GCRNN_ERR_UNSUPPORTED: a split batch keeps the state image


def test_scratch_switch_is_read_at_every_call(monkeypatch):
    """CPU: GCRNN_SEQ32_STATE_SCRATCH=0 / GCRNN_SEQ32P=1 select the state-image launch in the same process, at the next call."""
    from gated_gcrnns_amd import _lib
    q = _lib.lib.gcrnn_fused_forward_wide_scratch_bytes
    monkeypatch.delenv('GCRNN_SEQ32_STATE_SCRATCH', raising=False)
    monkeypatch.delenv('GCRNN_SEQ32P', raising=False)
    assert q(256, 64, 0) > 0
    monkeypatch.setenv('GCRNN_SEQ32_STATE_SCRATCH', '0')
    assert q(256, 64, 0) == -1
    monkeypatch.setenv('GCRNN_SEQ32_STATE_SCRATCH', '1')
    assert q(256, 64, 0) > 0
    monkeypatch.setenv('GCRNN_SEQ32P', '1')
    assert q(256, 64, 0) == -1
    monkeypatch.setenv('GCRNN_SEQ32P', '0')
    assert q(256, 64, 0) > 0


@pytest.mark.gpu
def test_scratch_entry_point_with_a_small_scratch_launches_nothing(monkeypatch):
    """GPU: with real arrays and a scratch one byte short the call returns the error code and H keeps the caller's bytes."""
    from gated_gcrnns_amd import _lib, ops
    N, F, G, K, B, T = 1000, 64, 64, 5, 4, 3
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    wide = ops.fused_wide_plan(cell.graph, B, T, N, F, G, K, False)
    assert wide is not None
    xs, hs_all = ops.fused_pack_inputs(Xd, hd, cell.graph)
    st = ops._stream()
    wpw = ops._fused_pack_weights_wide(cell.weight_A.detach(), cell.weight_B.detach(), wide['uniform_w'], st)
    need = int(_lib.lib.gcrnn_fused_forward_wide_scratch_bytes(B, F, 0))
    assert need == B * 65536
    scr = torch.empty((need,), dtype=torch.uint8, device=dev)
    H = torch.full((B, T, F, N), 7.0, dtype=torch.bfloat16, device=dev)
    p = ops._p
    b32 = cell.bias.detach().float().contiguous().view(-1)

    def call(nbytes):
        return _lib.lib.gcrnn_fused_forward_wide_scratch_bf16(p(xs), p(hs_all[:1]), p(scr), nbytes, p(wpw), p(b32), None, None, p(wide['tile_slots']),
                                                              p(wide['tile_off']), p(wide['ell_col4']), wide['entries'], B, T, N, F, G, K, p(H), 0, None,
                                                              None, None, st)
    assert call(need - 1) == 2
    torch.cuda.synchronize()
    assert bool((H == 7.0).all())
    assert call(need) == 0                                       # the same call with the bytes it asked for is the cell's forward
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(H, cell(Xd, hd))
