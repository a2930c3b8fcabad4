"""The chunk epilogue of the wide forward (csrc/gcrnn_fused_seq32.h): user-layout row stores with a static wave -> row mapping, and the next
chunk's seed taps evaluated beside them. Both move work and change no arithmetic, so H is pinned BIT for bit to the commit before
the change: tests/golden/wide_epilogue_digests.json holds the SHA-256 of H's bytes, recorded on an MI355X from a build of that commit (its hash
is in the file) with the inputs below. The kernel has no atomics and two calls give equal bits (tests/test_state_scratch.py). A wrong overlap
would give a plausible second chunk and the digests alone would not say which side is right: case 1 and the bench shape are also compared with
the fp64 oracle."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import gcrnn_oracle as orc
from test_wide import _normalized_adjacency, _uniform_cell, bf16_round

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wide_epilogue_digests.json')

# (N, F, G, K, B, T, what): each the smallest shape at which a branch of the epilogue can go wrong
#  1: segs = 125 -- a partial second sweep of the row stores; a chunk boundary with the overlapped seed taps
#  2: segs = 126, more sequences than CUs            3: exactly one sweep (segs = 64)
#  4: one segment; K = 2 keeps its end-of-chunk wait  5: F = 32, one chunk: no overlapped boundary
#  6: XS = 1                                          7: T = 1
#  8: case 1, the last state only                     9: case 1 on the normalised adjacency (rank-1 weights: the seed's put scales by a)
# 10: case 1 with time gates (another tap body: it keeps the seed behind the end barrier)
CASES = {
    'c01_n1000': (1000, 64, 64, 5, 4, 3, ''),
    'c02_n1008_b260': (1008, 64, 64, 5, 260, 2, ''),
    'c03_n512_k3': (512, 64, 64, 3, 4, 3, ''),
    'c04_n8_k2': (8, 64, 64, 2, 4, 3, ''),
    'c05_n200_f32': (200, 32, 32, 5, 4, 3, ''),
    'c06_g32_k4': (1000, 64, 32, 4, 4, 2, ''),
    'c07_t1': (1000, 64, 64, 5, 5, 1, ''),
    'c08_last_only': (1000, 64, 64, 5, 4, 3, 'last_only'),
    'c09_rank1': (1000, 64, 64, 5, 4, 3, 'rank1'),
    'c10_time_gated': (1000, 64, 64, 5, 4, 3, 'time_gated'),
}


def _problem(N, F, G, K, B, T, seed=89, dev=None, what=''):
    """Seeded as tests/test_wide_self_start.py::_problem; 'rank1' as its rank-1 test (seed 47)."""
    if what == 'rank1':
        import gated_gcrnns_amd.Utils.graphML as gml
        S, rng = _normalized_adjacency(N, 47, 'sym')
        torch.manual_seed(47)
        cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, False, None, 1, True)
        cell.addGSO(torch.tensor(S))
        cell = cell.to(torch.bfloat16)
    else:
        cell, rng, S = _uniform_cell(N, G, F, K, seed, time_gating=(what == 'time_gated'))
    X = bf16_round(rng.standard_normal((B, T, G, N)))
    h0 = bf16_round(0.3 * rng.standard_normal((B, F, N)))
    Xd = torch.tensor(X, dtype=torch.bfloat16, device=dev)
    hd = torch.tensor(h0, dtype=torch.bfloat16, device=dev)
    return cell, S, X, h0, Xd, hd


def digest(H):
    return hashlib.sha256(H.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def run_case(name, setenv):
    """H of a case under no_grad, as the module issues the forward. setenv(key, value) sets an environment variable for the caller's scope."""
    N, F, G, K, B, T, what = CASES[name]
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, dev=dev, what=what)
    cell = cell.to(dev)
    if B < 129:
        setenv('GCRNN_SEQ32_MIN_B', '1')      # (small batches: onto the persistent wide kernel, as tests/test_wide.py does)
    with torch.no_grad():
        H = cell(Xd, hd, **({'last_only': True} if what == 'last_only' else {}))
    torch.cuda.synchronize()
    assert tuple(H.shape) == (B, 1 if what == 'last_only' else T, F, N)
    return H, (cell, S, X, h0, Xd, hd)


_case1 = {}


def _case1_once(monkeypatch):
    """Case 1 is shared (digest, state image, capture, oracle): computed once, never modified."""
    monkeypatch.setenv('GCRNN_SEQ32_MIN_B', '1')
    if not _case1:
        H, prob = run_case('c01_n1000', monkeypatch.setenv)
        _case1['H'], _case1['prob'] = H.clone(), prob
    return _case1['H'], _case1['prob']


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_epilogue_bits_are_those_of_the_commit_before(case, monkeypatch):
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    H = _case1_once(monkeypatch)[0] if case == 'c01_n1000' else run_case(case, monkeypatch.setenv)[0]
    assert float(H.float().abs().max()) > 0.1                     # (not an all-zero tensor)
    d = digest(H)
    print('%s sha256 %s (recorded on %s: %s)' % (case, d, gold['commit'][:12], gold['digests'][case]))
    assert d == gold['digests'][case]


@pytest.mark.gpu
def test_state_image_launch_gives_the_same_bits(monkeypatch):
    """Case 11: return_states=True issues the launch WITH the state image (VAR 3: the training forward's, which shares the tanh and the row
    stores but not the state scratch) -- its user-layout H equals the no_grad call's, bit for bit."""
    from gated_gcrnns_amd import ops
    H, (cell, S, X, h0, Xd, hd) = _case1_once(monkeypatch)
    with torch.no_grad():
        hs_all, plan, H3 = ops.fused_cell_forward(Xd, hd, cell.weight_A, cell.weight_B, cell.bias, cell.graph, return_states=True)
    torch.cuda.synchronize()
    assert torch.equal(H3, H), float((H3.float() - H.float()).abs().max())


@pytest.mark.gpu
def test_captured_replay_equals_the_eager_call(monkeypatch):
    from gated_gcrnns_amd import ops
    H, (cell, S, X, h0, Xd, hd) = _case1_once(monkeypatch)
    with torch.no_grad():
        runner = ops.FusedForwardGraph(cell, Xd.shape[0], Xd.shape[1], X=Xd, h0=hd)
        assert torch.equal(runner(), H)
        assert torch.equal(runner(), H)


@pytest.mark.gpu
def test_case_1_matches_the_oracle(monkeypatch):
    """fp64 oracle on the bf16-rounded operands; tolerances of tests/test_wide_self_start.py's oracle test (5e-3 max, 1e-3 mean)."""
    H, (cell, S, X, h0, Xd, hd) = _case1_once(monkeypatch)
    params = {k: v.detach().double().cpu().numpy() for k, v in cell.state_dict().items()}
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X[:3], h0[:3])
    err = np.abs(H[:3].double().cpu().numpy() - Href)
    print('case 1 vs oracle: max %.3e mean %.3e' % (err.max(), err.mean()))
    assert err.max() <= 5.0e-3 and err.mean() <= 1.0e-3, (err.max(), err.mean())


@pytest.mark.gpu
def test_bench_shape_matches_the_oracle():
    """B = 256 (every workgroup of the chip runs), T = 4, against the dense fp64 oracle on three sequences; same tolerances."""
    N, F, G, K, B, T = 1000, 64, 64, 5, 256, 4
    dev = torch.device('cuda:0')
    cell, S, X, h0, Xd, hd = _problem(N, F, G, K, B, T, seed=73, dev=dev)
    params = {k: v.detach().double().numpy() for k, v in cell.state_dict().items()}
    pick = [0, 129, 255]
    Href = orc.ggcrnn_cell(params, S.astype(np.float32).astype(np.float64), X[pick], h0[pick])
    cell = cell.to(dev)
    with torch.no_grad():
        H = cell(Xd, hd)
    err = np.abs(H[pick].double().cpu().numpy() - Href)
    print('bench shape vs oracle, T = 4: max %.3e mean %.3e' % (err.max(), err.mean()))
    assert err.max() <= 5.0e-3 and err.mean() <= 1.0e-3, (err.max(), err.mean())
