"""GPU: the epicenter driver's loss and metric on the one-pass HIP kernel (gcrnn_cross_entropy): loss, gradient and argmax hit count
against torch.nn.functional.cross_entropy / torch.argmax evaluated in float64 on the host.

Bounds (the project's parity bounds, README's last table row): relative 1e-11 for fp64 and 1e-5 for fp32, on the loss and on the gradient
relative to its largest entry. bf16 logits are compared with the fp64 result on the SAME bf16-rounded logits: the loss at the fp32 bound
(the kernel accumulates in fp32 and returns the loss in fp32), a gradient entry within one bf16 ulp -- relative 2^-7 of the entry (fp32
arithmetic, then one rounding that the fp32 error may tip), plus 2^-8 * inv_B absolute for the cancelling entry at the label
(softmax - 1 cancels to a small number whose fp32 error is relative to 1, not to the entry). Where the largest gradient entry is 0 (C = 1) the
bound is absolute: the same figure times inv_B. Hit counts are compared exactly, in every case: the kernel reads the stored values
torch.argmax reads."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DTYPES = {'f64': torch.float64, 'f32': torch.float32, 'bf16': torch.bfloat16}
REL = {'f64': 1e-11, 'f32': 1e-5, 'bf16': 1e-5}
SHAPES = [(1, 1), (1, 11), (3, 2), (100, 11), (257, 64), (64, 1000)]


def _problem(B, C, dt, seed):
    """logits N(0, 3^2) in `dt` with some rows carrying one logit at +80 or -80 (the maximum must be subtracted), labels uniform."""
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(B, C, dtype=torch.float64, generator=g)
    for r in range(0, B, 3):
        z[r, int(torch.randint(0, C, (1,), generator=g))] = 80.0 if (r // 3) % 2 == 0 else -80.0
    lab = torch.randint(0, C, (B,), generator=g)
    return z.to(dt), lab


def _host_reference(z, lab):
    """fp64 on the host from the values the kernel reads: loss, gradient, hits."""
    z64 = z.detach().cpu().to(torch.float64).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(z64, lab.cpu())
    loss.backward()
    hits = int((torch.argmax(z64.detach(), dim=1) == lab.cpu()).sum())
    return float(loss.detach()), z64.grad.numpy(), hits


def _check(tag, z, lab, loss, grad, hits):
    B = z.shape[0]
    ref_loss, ref_grad, ref_hits = _host_reference(z, lab)
    got = grad.detach().cpu().to(torch.float64).numpy()
    el = abs(float(loss.detach()) - ref_loss)
    big = np.max(np.abs(ref_grad))
    if tag == 'bf16':
        bound = 2.0 ** -7 * np.abs(ref_grad) + 2.0 ** -8 / B
        eg = float(np.max(np.abs(got - ref_grad) - bound))                     # <= 0 passes
        gb = 0.0
    else:
        eg = float(np.max(np.abs(got - ref_grad)))
        gb = REL[tag] * big if big > 0 else REL[tag] / B
    print('%s B=%d C=%d: loss %.12g ref %.12g |d| %.3g (bound %.3g); grad err %.3g (bound %.3g, max entry %.3g); hits %d ref %d'
          % (tag, B, z.shape[1], float(loss.detach()), ref_loss, el, REL[tag] * abs(ref_loss), eg, gb, big, int(hits), ref_hits))
    assert int(hits) == ref_hits
    assert el <= REL[tag] * abs(ref_loss)
    assert eg <= gb


def _check_accuracy(acc, hits, B):
    """hits / B: one division in the result type (the device may form it as hits * (1 / B): two roundings, each half an ulp of a value <= 1)."""
    eps = 2.0 ** -52 if acc.dtype == torch.float64 else 2.0 ** -23
    assert abs(float(acc) - hits / B) <= eps and round(float(acc) * B) == hits


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('tag', ['f64', 'f32', 'bf16'])
def test_loss_gradient_hits_match_host_fp64(tag, shape):
    from gated_gcrnns_amd import ops
    B, C = shape
    z, lab = _problem(B, C, DTYPES[tag], 100 * B + C)
    zd = z.to(DEV).requires_grad_(True)
    loss, hits = ops.cross_entropy(zd, lab.to(DEV), return_hits=True)
    loss.backward()
    assert loss.dtype == (torch.float64 if tag == 'f64' else torch.float32) and zd.grad.dtype == DTYPES[tag]
    assert hits.dtype == torch.int64 and hits.is_cuda and hits.dim() == 0
    _check(tag, z, lab, loss, zd.grad, hits)
    acc = ops.accuracy(zd.detach(), lab.to(DEV))
    assert acc.dtype == (torch.float64 if tag == 'f64' else torch.float32) and acc.is_cuda and acc.dim() == 0
    _check_accuracy(acc, int(hits), B)
    # labels as the dataset keeps them: in the data type, B x 1
    if tag != 'bf16':
        loss2, hits2 = ops.cross_entropy(zd.detach(), lab.to(DEV, DTYPES[tag]).reshape(B, 1), return_hits=True)
        assert torch.equal(loss2, loss.detach()) and int(hits2) == int(hits)


@pytest.mark.parametrize('tag', ['f64', 'f32', 'bf16'])
def test_ties_hit_only_at_the_first_maximal_index(tag):
    from gated_gcrnns_amd import ops
    dt = DTYPES[tag]
    for C in (2, 11, 64, 65, 300):
        rows, labs, want = [], [], 0
        for lab in range(min(C, 4)):
            rows.append(torch.full((C,), 1.5))                                  # all equal: argmax = 0
            labs.append(lab)
            want += lab == 0
        a, b = 1 % C, C - 1                                                      # the maximum occurs at a and again at b > a
        if b > a:
            for lab in (a, b, 0):
                r = torch.zeros(C)
                r[a] = r[b] = 2.0
                rows.append(r)
                labs.append(lab)
                want += lab == a
        z = torch.stack(rows).to(dt)
        lab = torch.tensor(labs)
        _, hits = ops.cross_entropy(z.to(DEV), lab.to(DEV), return_hits=True)
        assert int(hits) == want == int((torch.argmax(z, dim=1) == lab).sum()), (C, int(hits), want)
        _check_accuracy(ops.accuracy(z.to(DEV), lab.to(DEV)), want, len(labs))


@pytest.mark.parametrize('tag', ['f64', 'f32', 'bf16'])
def test_out_of_range_labels_give_nan_rows_and_touch_nothing_else(tag):
    from gated_gcrnns_amd import ops
    B, C = 37, 11
    z, lab = _problem(B, C, DTYPES[tag], 7)
    bad = {2: -100, 5: -1, 36: C}
    labb = lab.clone()
    for r, v in bad.items():
        labb[r] = v
    zg = z.to(DEV).requires_grad_(True)
    ops.cross_entropy(zg, lab.to(DEV)).backward()
    zb = z.to(DEV).requires_grad_(True)
    loss, hits = ops.cross_entropy(zb, labb.to(DEV), return_hits=True)
    loss.backward()
    assert bool(torch.isnan(loss))
    good = torch.tensor([r not in bad for r in range(B)])
    assert bool(torch.isnan(zb.grad[~good.to(DEV)]).all())
    assert torch.equal(zb.grad[good.to(DEV)], zg.grad[good.to(DEV)])               # in-range rows: the same bits
    assert int(hits) == int((torch.argmax(z, dim=1) == lab)[good].sum())
    _check_accuracy(ops.accuracy(z.to(DEV), labb.to(DEV)), int(hits), B)


@pytest.mark.parametrize('tag', ['f64', 'f32', 'bf16'])
def test_repeatable_upstream_double_backward_and_fallback(tag):
    from gated_gcrnns_amd import ops
    dt = DTYPES[tag]
    B, C = 257, 64
    z, lab = _problem(B, C, dt, 11)
    labd = lab.to(DEV)
    runs = []
    for _ in range(2):
        zd = z.to(DEV).requires_grad_(True)
        loss, hits = ops.cross_entropy(zd, labd, return_hits=True)
        loss.backward()
        runs.append((loss.detach().clone(), hits.clone(), zd.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))                        # bit for bit
    loss1, _, g1 = runs[0]
    # upstream 0.5: a power of two scales exactly
    zd = z.to(DEV).requires_grad_(True)
    (0.5 * ops.cross_entropy(zd, labd)).backward()
    # (exactly for every normal number; an entry in the subnormal range -- softmax tails next to a logit at +80 -- may lose its last bit)
    assert float((zd.grad.to(torch.float64) - 0.5 * g1.to(torch.float64)).abs().max()) <= (0.0 if tag == 'f64' else 2.0 ** -126)
    # double backward over a retained graph: the second gets a fresh gradient, the leaf accumulates both
    zd = z.to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(zd, labd)
    loss.backward(retain_graph=True)
    first = zd.grad.clone()
    loss.backward()
    assert torch.equal(first, g1)
    assert torch.equal(zd.grad.to(torch.float64), (g1 + g1).to(torch.float64))
    # more classes than the kernel takes: torch's own expressions, never an error
    Cb = ops.CROSS_ENTROPY_MAX_CLASSES + 1
    zb, lb = _problem(5, Cb, dt, 13)
    assert not ops.cross_entropy_supported(zb.to(DEV)) and ops.cross_entropy_supported(z.to(DEV))
    zd = zb.to(DEV).requires_grad_(True)
    loss, hits = ops.cross_entropy(zd, lb.to(DEV), return_hits=True)
    loss.backward()
    zt = zb.to(DEV).requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(zt, lb.to(DEV))
    lt.backward()
    assert torch.equal(loss.detach(), lt.detach()) and torch.equal(zd.grad, zt.grad)
    assert int(hits) == int((torch.argmax(zb, dim=1) == lb).sum())
    _check_accuracy(ops.accuracy(zb.to(DEV), lb.to(DEV)), int(hits), 5)
    # a non-contiguous view is made contiguous
    zw = torch.cat([z, z], dim=1).to(DEV)[:, :C]
    assert not zw.is_contiguous()
    assert torch.equal(ops.cross_entropy(zw, labd), loss1)


@pytest.mark.parametrize('tag', ['f64', 'f32'])
def test_captured_forward_backward_replays_the_eager_bits(tag):
    from gated_gcrnns_amd import ops
    dt = DTYPES[tag]
    B, C = 100, 11
    z0, lab0 = _problem(B, C, dt, 21)
    zs = z0.to(DEV).requires_grad_(True)
    ls = lab0.to(DEV)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        for _ in range(2):
            zs.grad = None
            ops.cross_entropy(zs, ls).backward()
    torch.cuda.current_stream(DEV).wait_stream(s)
    zs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        loss_s, hits_s = ops.cross_entropy(zs, ls, return_hits=True)
        loss_s.backward()
    for seed in (22, 23):
        z1, lab1 = _problem(B, C, dt, seed)
        with torch.no_grad():
            zs.copy_(z1.to(DEV))
        ls.copy_(lab1.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        ze = z1.to(DEV).requires_grad_(True)
        le, he = ops.cross_entropy(ze, lab1.to(DEV), return_hits=True)
        le.backward()
        assert torch.equal(loss_s.detach(), le.detach()) and torch.equal(hits_s, he) and torch.equal(zs.grad, ze.grad)
