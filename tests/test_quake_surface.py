"""CPU: the epicenter-estimation driver's surface without a GPU -- Utils/dataTools.QuakeData against the reference class (golden
g18_quake_data: the same arrays under the same numpy seed, tests/golden/make_golden_quake.py), the host fallbacks of the cross-entropy loss
and the accuracy, the C entry's argument checks, and Modules/train_rnn_quake.MultipleModels over two gloo ranks."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_golden


def _dataset(d, **kw):
    from gated_gcrnns_amd.Utils.dataTools import QuakeData
    np.random.seed(int(d['seed']))
    return QuakeData(int(d['nTrain']), int(d['nValid']), int(d['nTest']), int(d['seqLen']), int(d['downsamplingFactor']),
                     X=d['X'], y=d['y'], **kw)


def test_quake_data_reproduces_the_reference_split_window_and_samples():
    d = load_golden('g18_quake_data')
    data = _dataset(d, dataType=torch.float64)
    assert (data.nTrain, data.nValid, data.nTest) == (18, 6, 4)
    for split in ('train', 'valid', 'test'):
        x, y = data.getSamples(split)
        assert x.dtype == torch.float64 and y.dtype == torch.float64 and tuple(y.shape) == (x.shape[0], 1)
        assert np.array_equal(x.numpy(), d[split + '_signals']) and np.array_equal(y.numpy(), d[split + '_labels'])
        assert np.array_equal(data.samples[split]['signals'].numpy(), d[split + '_signals'])
    # the window: samples 0, 2, ..., 38 of a 41-sample recording (X[:, -2000:-1:2, :]), flattened sample-major
    assert tuple(data.getSamples('train')[0].shape) == (18, 20 * 59)
    x, y = data.getSamples('train', [3, 1, 4])
    assert np.array_equal(x.numpy(), d['pick_list_signals']) and np.array_equal(y.numpy(), d['pick_list_labels'])
    x1, _ = data.getSamples('train', [2])
    assert tuple(x1.shape) == (1, 20 * 59)
    np.random.seed(181)
    x, y = data.getSamples('valid', 3)
    assert np.array_equal(x.numpy(), d['pick_int_signals']) and np.array_equal(y.numpy(), d['pick_int_labels'])
    # evaluate on host tensors
    yv = data.getSamples('valid')[1]
    acc = data.evaluate(torch.tensor(d['eval_logits']), yv.squeeze())
    assert float(acc) == float(d['eval_accuracy'])
    assert float(data.evaluate(torch.tensor(d['eval_logits']), yv)) == float(d['eval_accuracy'])         # n x 1 labels are squeezed
    # numpy data type, and astype / to afterwards
    dn = _dataset(d)
    assert isinstance(dn.samples['train']['signals'], np.ndarray) and np.array_equal(dn.getSamples('test')[0], d['test_signals'])
    assert float(dn.evaluate(d['eval_logits'], dn.getSamples('valid')[1].squeeze())) == float(d['eval_accuracy'])
    dn.astype(torch.float32)
    dn.to('cpu')
    assert dn.samples['valid']['labels'].dtype == torch.float32 and dn.dataType is torch.float32
    with pytest.raises(AssertionError):
        data.getSamples('nope')


def test_synthetic_waves_moved_with_the_same_draws():
    """examples/epicenter_estimation.py imports the generator from dataTools: the same generator calls in the same order."""
    from gated_gcrnns_amd.Utils import dataTools
    S = load_golden('g18_quake_data')['S'][0]
    regions = (np.arange(59) * 11) // 59
    x, y = dataTools.synthetic_waves(S, 7, 20, regions, np.random.default_rng(0))
    rng = np.random.default_rng(0)
    src = rng.integers(0, 59, size=7)
    t0 = rng.integers(8, 17, size=7)
    noise = 0.02 * rng.standard_normal((7, 20, 59))
    assert x.shape == (7, 20, 59) and np.array_equal(y, regions[src])
    assert np.array_equal(x[:, :int(t0.min())], noise[:, :int(t0.min())])      # nothing but noise before the first pulse


def test_host_fallbacks_equal_torch():
    from gated_gcrnns_amd.Utils.miscTools import CrossEntropyLoss, accuracy, crossEntropyLoss
    g = torch.Generator().manual_seed(0)
    z = torch.randn(9, 11, dtype=torch.float64, generator=g).requires_grad_(True)
    lab = torch.randint(0, 11, (9,), generator=g)
    zr = z.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(zr, lab)
    ref.backward()
    for y in (lab, lab.to(torch.float64).reshape(9, 1)):                 # int64, or the dataset's floating n x 1 labels
        z.grad = None
        loss_fn = CrossEntropyLoss()
        loss = loss_fn(z, y)
        loss.backward()
        assert torch.equal(loss.detach(), ref.detach()) and torch.equal(z.grad, zr.grad)
        hits = int((z.detach().argmax(dim=1) == lab).sum())
        assert int(loss_fn.last_hits) == hits and loss_fn.last_count == 9
        assert float(accuracy(z.detach(), y)) == 1 - (9 - hits) / 9
    assert isinstance(crossEntropyLoss, CrossEntropyLoss)
    assert accuracy(z.detach().float(), lab).dtype == torch.float32


def test_cross_entropy_entry_checks_arguments_before_any_launch():
    from gated_gcrnns_amd import _lib, ops
    lib = _lib.lib
    one = C.c_void_p(16)
    assert lib.gcrnn_cross_entropy_blocks(100, 11) == 25 and lib.gcrnn_cross_entropy_blocks(1, 1) == 1
    assert lib.gcrnn_cross_entropy_blocks(10 ** 6, 64) == 2048
    assert lib.gcrnn_cross_entropy_blocks(8, ops.CROSS_ENTROPY_MAX_CLASSES) == 2
    assert lib.gcrnn_cross_entropy_blocks(8, ops.CROSS_ENTROPY_MAX_CLASSES + 1) == 0 and lib.gcrnn_cross_entropy_blocks(0, 4) == 0
    assert lib.gcrnn_cross_entropy(0, None, one, None, one, one, one, one, 4, 4, 0.25, None) == 3
    assert lib.gcrnn_cross_entropy(0, one, one, None, one, one, one, None, 4, 4, 0.25, None) == 3
    assert lib.gcrnn_cross_entropy(0, one, one, None, one, one, one, one, 0, 4, 0.25, None) == 2
    assert lib.gcrnn_cross_entropy(0, one, one, None, one, one, one, one, 4, 1025, 0.25, None) == 4     # GCRNN_ERR_UNSUPPORTED
    assert lib.gcrnn_cross_entropy(7, one, one, None, one, one, one, one, 4, 4, 0.25, None) == 1
    with pytest.raises(_lib.GcrnnError, match='no CPU path'):
        ops.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class TinyClassifier(torch.nn.Module):
    """CPU stand-in with the surface the harness touches for a name with 'GCRNN': archit.stateGCRNN.weight_A, archit(x, h0) -> logits."""

    def __init__(self, N, classes):
        super().__init__()
        self.stateGCRNN = torch.nn.Module()
        self.stateGCRNN.weight_A = torch.nn.Parameter(torch.randn(N, classes, dtype=torch.float64) * 0.3)

    def forward(self, x, h0):                       # x: B x T x 1 x N -> the last sample's projection
        return torch.tanh(x[:, -1, 0]) @ self.stateGCRNN.weight_A + 0.0 * h0.sum()


def harness_worker(rank, world, port, ret, save_dir):
    """train_rnn_quake.MultipleModels over two ranks with the shared crossEntropyLoss on CPU tensors (its torch fallback): unequal shards
    (batches of 5 = 3 + 2) and a last global batch of ONE sample that leaves rank 1 empty. Both ranks must end with identical parameters,
    equal to a single process that trains on the whole batches."""
    from gated_gcrnns_amd.Modules.train_rnn_quake import MultipleModels, TrainableModel
    from gated_gcrnns_amd.optim import FlatAdam
    from gated_gcrnns_amd.Utils.miscTools import accuracy, crossEntropyLoss
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    N, T, nTrain, bs, classes = 6, 3, 11, 5, 4        # batches of 5, 5, 1
    g = torch.Generator().manual_seed(3)
    xT = torch.randn(nTrain, T * N, dtype=torch.float64, generator=g)
    yT = torch.randint(0, classes, (nTrain, 1), generator=g).to(torch.float64)      # the dataset's form: n x 1 in the data type
    xV = torch.randn(4, T * N, dtype=torch.float64, generator=g)
    yV = torch.randint(0, classes, (4, 1), generator=g).to(torch.float64)

    def build(d):
        torch.manual_seed(5)
        m = TinyClassifier(N, classes)
        return m, TrainableModel(m, crossEntropyLoss, FlatAdam(m.parameters(), lr=1e-2), 'TinyGCRNN', d)

    mdl, tm = build(save_dir)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    kw = dict(nEpochs=2, batchSize=bs, seqLen=T, stateFeat=2, evaluate=accuracy, validationInterval=2)
    out = MultipleModels({'TinyGCRNN': tm}, xT, yT, xV, yV, rank=rank, world=world, rng=np.random.RandomState(11), **kw)
    mine = mdl.stateGCRNN.weight_A.detach().reshape(-1).clone()
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    ok = all(torch.equal(t, gathered[0]) for t in gathered)
    dist.destroy_process_group()
    ok &= len(out['lossTrain']['TinyGCRNN']) == 6 and len(out['evalValid']['TinyGCRNN']) == 3
    ok &= os.path.exists(os.path.join(save_dir, 'savedModels', 'TinyGCRNNArchitBest.ckpt'))        # (written by rank 0 before the all_gather)
    ref, rtm = build(os.path.join(save_dir, 'single'))
    rout = MultipleModels({'TinyGCRNN': rtm}, xT, yT, xV, yV, rng=np.random.RandomState(11), **kw)
    ok &= bool(torch.allclose(mine, ref.stateGCRNN.weight_A.detach().reshape(-1), atol=1e-12, rtol=0))
    ok &= rout['evalValid']['TinyGCRNN'] == out['evalValid']['TinyGCRNN']          # every rank validates on the whole validation set
    ret[rank] = bool(ok)


def test_quake_harness_world2_keeps_replicas_identical(tmp_path):
    world = 2
    port = free_port()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(harness_worker, args=(world, port, ret, str(tmp_path)), nprocs=world, join=True)
    assert all(ret[r] for r in range(world)), dict(ret)
