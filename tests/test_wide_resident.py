"""Resident tiles of the wide inference forward (csrc/gcrnn_fused_seq32.h, template argument RT; instantiated in csrc/gcrnn_fused_seq32r.hip):
the un-gated forward as the module issues it (inline pack, user-layout H, state scratch) at F = 64 keeps the tap weights in a ring of three
taps and, in the LDS bytes that frees, the chunk-0 state fragment of every wave's first three (or two) tiles -- those 16 bytes per lane and tile go
from the epilogue that makes them to the next step's operand through a wave-private LDS block instead of the state scratch. Bytes move, no
arithmetic does: H is BIT-identical to the launch without them (GCRNN_SEQ32_RESIDENT=0, read by the library at every call) and to the
state-image launch (ops.fused_cell_forward(..., return_states=True)), which tests/test_wide.py and tests/test_state_scratch.py pin to the
fp64 oracle; one case here is held to the oracle directly.

Which launch ran: gcrnn_fused_forward_wide_resident_tiles answers what the host dispatch asks (3, 2 where the map has no room for the
third tile or with GCRNN_SEQ32_RESIDENT=2, 0 with the switch off / at F = 32), and the forward entry point is counted with its self-start flag as tests/test_wide_self_start.py does."""
import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from test_wide import _normalized_adjacency, _uniform_cell, bf16_round

_FWD = 'gcrnn_fused_forward_wide_scratch_bf16'


def _count_forward(monkeypatch):
    """Calls of the state-scratch entry point, and how many of them carried GCRNN_WIDE_SELF_START (argument 19)."""
    from gated_gcrnns_amd import _lib
    n = {'fwd': 0, 'self': 0}
    orig = getattr(_lib.lib, _FWD)

    def wrapped(*a):
        n['fwd'] += 1
        n['self'] += 1 if (int(a[19]) & 2) else 0
        return orig(*a)
    monkeypatch.setattr(_lib.lib, _FWD, wrapped, raising=False)
    return n


def _tiles(cell, B, T, N, F, G, K, rank1=False):
    from gated_gcrnns_amd import _lib, ops
    wide = ops.fused_wide_plan(cell.graph, B, T, N, F, G, K, True, rank1=rank1)
    assert wide is not None
    return int(_lib.lib.gcrnn_fused_forward_wide_resident_tiles(F, G, K, int(wide['entries']), 1 if rank1 else 0))


def _three_launches(cell, Xd, hd, monkeypatch, want_tiles=3, rank1=False):
    """H of the resident launch, of the same binary's launch with the switch off, and of the state-image launch. Where the launch keeps
    three tiles, the two-tile launch (GCRNN_SEQ32_RESIDENT=2) is run and compared here as well."""
    from gated_gcrnns_amd import ops
    B, T, G, N = Xd.shape
    F = hd.shape[1]
    K = cell.weight_A.shape[2]
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')              # (small batches: onto the persistent wide kernel, as tests/test_wide.py does)
    monkeypatch.delenv('GCRNN_SEQ32_RESIDENT', raising=False)
    assert _tiles(cell, B, T, N, F, G, K, rank1) == want_tiles
    n = _count_forward(monkeypatch)
    with torch.no_grad():
        H = cell(Xd, hd)
        torch.cuda.synchronize()
        assert n == {'fwd': 1, 'self': 1}, n                     # ONE launch, the self-start form: the one the resident tiles live in
        if want_tiles == 3:
            monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '2')
            assert _tiles(cell, B, T, N, F, G, K, rank1) == 2
            H2 = cell(Xd, hd)
            torch.cuda.synchronize()
            assert torch.equal(H, H2), float((H.float() - H2.float()).abs().max())
            n['fwd'] -= 1; n['self'] -= 1
        monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '0')
        assert _tiles(cell, B, T, N, F, G, K, rank1) == 0
        Hoff = cell(Xd, hd)
        torch.cuda.synchronize()
        assert n == {'fwd': 2, 'self': 2}, n
        monkeypatch.delenv('GCRNN_SEQ32_RESIDENT')
        _, _, Himg = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, return_states=True)
        torch.cuda.synchronize()
        assert n == {'fwd': 2, 'self': 2}, n                     # (the state-image launch is another entry point)
    return H, Hoff, Himg


def _problem(N, F, G, K, B, T, seed=101, dev=None):
    cell, rng, S = _uniform_cell(N, G, F, K, seed)
    X = bf16_round(rng.standard_normal((B, T, G, N)))
    h0 = bf16_round(0.3 * rng.standard_normal((B, F, N)))      # h0 != 0: a stale or zeroed block cannot pass for the state
    Xd = torch.tensor(X, dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(h0, dtype=torch.bfloat16, device=dev)
    return cell, S, X, h0, Xd, hd


# (N, F, G, K, B, T). T = 1: no reload; T = 2: the first reload; T = 4: the block and every ring slot re-used (K = 5: the ring wraps twice
# inside a chunk; K = 2: two items per chunk, both brought by the one hop; K = 3: 6 items per step = two turns of the ring, K = 5: 10 items,
# so the slot of a tap changes from step to step). N = 40: all but three tiles are padding slots, which store and reload their zeros;
# N = 992: the last tile is partly padding; N = 1000: the bench plan. G = 32: KS = 3, a tap is 6 KB and the block starts at another offset.
# B = 1 and 3; 'second_wg': four sequences more than CUs at T = 2 -- their workgroups start on CUs whose LDS holds another sequence's block.
CASES = {
    'k5_t1': (1000, 64, 64, 5, 3, 1),
    'k5_t2': (1000, 64, 64, 5, 3, 2),
    'k5_t4': (1000, 64, 64, 5, 3, 4),
    'k5_t4_b1': (1000, 64, 64, 5, 1, 4),
    'k3_t4': (1000, 64, 64, 3, 3, 4),
    'k3_t2_b1': (1000, 64, 64, 3, 1, 2),
    'k2_t4': (1000, 64, 64, 2, 3, 4),
    'k2_t1_b1': (1000, 64, 64, 2, 1, 1),
    'g32_k5_t4': (1000, 64, 32, 5, 3, 4),
    'g32_k3_t2': (1000, 64, 32, 3, 1, 2),
    'g32_k2_t4': (992, 64, 32, 2, 3, 4),
    'n40_k5_t4': (40, 64, 64, 5, 3, 4),
    'n40_k2_t2': (40, 64, 64, 2, 1, 2),
    'n40_g32_k3_t4': (40, 64, 32, 3, 3, 4),
    'n992_k5_t4': (992, 64, 64, 5, 3, 4),
    'n992_k3_t1': (992, 64, 64, 3, 1, 1),
    'second_wg': (1000, 64, 64, 5, -4, 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_resident_tiles_are_bit_identical_to_the_scratch_and_state_image_launches(case, monkeypatch):
    N, F, G, K, B, T = CASES[case]
    dev = torch.device('cuda:0')
    if B < 0:
        B = torch.cuda.get_device_properties(dev).multi_processor_count - B
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    H, Hoff, Himg = _three_launches(cell, Xd, hd, monkeypatch)
    assert tuple(H.shape) == (B, T, F, N)
    assert torch.equal(H, Hoff), float((H.float() - Hoff.float()).abs().max())
    assert torch.equal(H, Himg), float((H.float() - Himg.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1                     # (not three all-zero tensors)


@pytest.mark.gpu
def test_resident_tiles_match_the_oracle(monkeypatch):
    """The resident launch against the fp64 oracle at the tolerances tests/test_wide.py holds this kernel to at (1000, 64, 64, 5), T = 4:
    4e-3 at step 0, 5e-3 over all steps, 1e-3 mean."""
    N, F, G, K, B, T = 1000, 64, 64, 5, 3, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, seed=71, dev=dev)
    params = {k: v.detach().double().numpy() for k, v in cell.state_dict().items()}
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X, h0)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    monkeypatch.delenv('GCRNN_SEQ32_RESIDENT', raising=False)
    assert _tiles(cell, B, T, N, F, G, K) == 3
    n = _count_forward(monkeypatch)
    with torch.no_grad():
        H = cell(Xd, hd)
    assert n == {'fwd': 1, 'self': 1}, n
    err = np.abs(H.double().cpu().numpy() - Href)
    print('resident tiles vs oracle, T = 4: max %.3e mean %.3e (step 0: max %.3e)' % (err.max(), err.mean(), err[:, 0].max()))
    assert err[:, 0].max() <= 4.0e-3, err[:, 0].max()
    assert err.max() <= 5.0e-3 and err.mean() <= 1.0e-3, (err.max(), err.mean())


@pytest.mark.gpu
@pytest.mark.parametrize('kind,K,G,tiles', [('sym', 5, 64, 2), ('rw', 3, 64, 2), ('sym', 2, 32, 3)])
def test_resident_tiles_on_rank1_weighted_graphs_are_bit_identical(kind, K, G, tiles, monkeypatch):
    """Normalised adjacencies (the R1 instantiations: the factor tables lie between the slot table and the pack tile, above the block --
    at G = 64 they leave room for two tiles, not three)."""
    import gated_gcrnns_amd.Utils.graphML as gml
    dev = torch.device('cuda:0')
    N, F, B, T = 1000, 64, 3, 4
    S, rng = _normalized_adjacency(N, 53, kind)
    torch.manual_seed(53)
    cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, False, None, 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.to(torch.bfloat16).to(dev)
    Xd = torch.tensor(bf16_round(rng.standard_normal((B, T, G, N))), dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(bf16_round(0.3 * rng.standard_normal((B, F, N))), dtype=torch.bfloat16, device=dev)
    H, Hoff, Himg = _three_launches(cell, Xd, hd, monkeypatch, want_tiles=tiles, rank1=True)
    assert torch.equal(H, Hoff), float((H.float() - Hoff.float()).abs().max())
    assert torch.equal(H, Himg), float((H.float() - Himg.float()).abs().max())
    assert float(H.float().abs().max()) > 0.1


@pytest.mark.gpu
def test_one_chunk_states_keep_the_launch_as_it_was(monkeypatch):
    """F = 32: the state never leaves the registers, nothing is re-read, nothing is resident -- the query says 0 with either setting of the
    switch and the launch is the one it was."""
    N, F, G, K, B, T = 1000, 32, 32, 5, 3, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    H, Hoff, Himg = _three_launches(cell, Xd, hd, monkeypatch, want_tiles=0)
    assert torch.equal(H, Hoff) and torch.equal(H, Himg)
    assert float(H.float().abs().max()) > 0.1


@pytest.mark.gpu
def test_resident_tiles_replay_bit_identically(monkeypatch):
    """A FusedForwardGraph captured on the resident launch replays the eager call's bits, twice in a row (a replay finds the previous one's
    block and ring in LDS: step 0 reads neither) and after the caller refills X in place."""
    from gated_gcrnns_amd import ops
    N, F, G, K, B, T = 1000, 64, 64, 5, 3, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    monkeypatch.delenv('GCRNN_SEQ32_RESIDENT', raising=False)
    assert _tiles(cell, B, T, N, F, G, K) == 3
    with torch.no_grad():
        He = cell(Xd, hd).clone()
        runner = ops.FusedForwardGraph(cell, B, T, X=Xd, h0=hd)
        H1 = runner().clone()
        H2 = runner().clone()
        assert torch.equal(He, H1) and torch.equal(He, H2)
        Xd.copy_(torch.randn(B, T, G, N, device=dev).to(torch.bfloat16))
        H3 = runner().clone()
        monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '0')
        assert torch.equal(cell(Xd, hd), H3) and not torch.equal(H3, He)


@pytest.mark.gpu
def test_a_nan_input_stays_in_its_sequence_and_step(monkeypatch):
    """A NaN in X[b, t] of ONE sequence: the block is private to a workgroup's waves and a workgroup runs one sequence, so every other
    sequence, and the steps before t of the poisoned one, keep the bits of the clean run."""
    N, F, G, K, B, T = 1000, 64, 64, 5, 3, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev)
    cell = cell.to(dev)
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    monkeypatch.delenv('GCRNN_SEQ32_RESIDENT', raising=False)
    assert _tiles(cell, B, T, N, F, G, K) == 3
    bad_b, bad_t = 1, 2
    Xn = Xd.clone()
    Xn[bad_b, bad_t, 5, 17] = float('nan')
    with torch.no_grad():
        Hc = cell(Xd, hd)
        Hn = cell(Xn, hd)
    assert bool(torch.isnan(Hn[bad_b, bad_t:].float()).any())       # (the NaN did reach the state of its own sequence)
    for b in range(B):
        if b != bad_b:
            assert torch.equal(Hn[b], Hc[b]), b
    assert torch.equal(Hn[bad_b, :bad_t], Hc[bad_b, :bad_t])
    assert not bool(torch.isnan(Hc.float()).any())


def test_resident_switch_is_read_at_every_call(monkeypatch):
    """CPU: the query follows GCRNN_SEQ32_RESIDENT within one process, and says 0 where there is no such launch or no LDS room."""
    from gated_gcrnns_amd import _lib
    q = _lib.lib.gcrnn_fused_forward_wide_resident_tiles
    assert 'gcrnn_fused_forward_wide_resident_tiles' in _lib.EXPORTS
    monkeypatch.delenv('GCRNN_SEQ32_RESIDENT', raising=False)
    for K in (2, 3, 4, 5):
        for G in (32, 64):
            assert q(64, G, K, 732, 0) == 3
            assert q(64, G, K, 732, 1) == ((0 if K == 4 else 2) if G == 64 else 3)      # (G = 64: no room for the third tile beside the factor tables; K = 4 there: that one instantiation would spill and keeps RT = 0)
    assert q(32, 32, 5, 732, 0) == 0 and q(64, 48, 5, 732, 0) == 0 and q(64, 64, 6, 732, 0) == 0
    assert q(64, 64, 5, 4000, 0) == 0                            # the column words of such a graph leave no room at all
    monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '0')
    assert q(64, 64, 5, 732, 0) == 0
    monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '2')
    assert q(64, 64, 5, 732, 0) == 2
    monkeypatch.setenv('GCRNN_SEQ32_RESIDENT', '1')
    assert q(64, 64, 5, 732, 0) == 3
    assert q(64, 64, 5, 1000, 0) == 2 and q(64, 64, 5, 1100, 0) == 0      # (more column words: first the third tile goes, then the block)
