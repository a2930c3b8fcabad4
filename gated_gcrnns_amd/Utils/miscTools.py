"""Losses / metrics of the training loops: the k-step drivers' (counterpart of the reference's Utils/miscTools.py:112-130) and the
epicenter-estimation driver's (nn.CrossEntropyLoss(), epicenterEstimation.py:117; QuakeData.evaluate, Utils/dataTools.py:1564-1586)."""
import torch


def batchTimeL1Loss(x, y):
    """Mean absolute error over every entry (reference miscTools.py:112-119; its view(-1,N,F) is a no-op for a mean)."""
    from .. import ops
    y = y.to(x.dtype)
    if x.shape != y.shape:
        x, y = torch.broadcast_tensors(x, y)
    return ops.l1_loss(x, y)


def batchTimeMSELoss(x, y):
    """Per flattened (N*F) column: sqrt(sum_rows (x-y)^2) / ||y column||_2, averaged over columns
    (reference miscTools.py:121-130). A metric (the drivers never back-propagate it): on the device without autograd it is
    two launches (gcrnn_batch_time_mse: column partial sums over row slabs, fixed-order finish); anything that needs a
    gradient takes the torch expression."""
    F, N = x.shape[-2], x.shape[-1]
    xv = x.reshape(-1, N * F)
    yv = y.to(x.dtype).reshape(-1, N * F)
    if x.is_cuda and not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)) and \
            x.dtype in (torch.float32, torch.float64, torch.bfloat16):
        from .. import ops
        return ops.batch_time_mse(xv.contiguous(), yv.contiguous())
    num = torch.sqrt(torch.sum((xv - yv) ** 2, dim=0))
    return torch.mean(num / torch.norm(yv, dim=0))


def _labels(y, B):
    return y.reshape(-1).to(torch.int64) if y.numel() == B else y.to(torch.int64)


class CrossEntropyLoss(object):
    """The epicenter driver's `lossFunction` (nn.CrossEntropyLoss() with its defaults: mean over the batch, no class weights, and NO
    ignore_index: a label outside [0, C) gives NaN on the device) on ops.cross_entropy: loss, gradient and argmax hit count from one
    kernel launch. After a call, `last_hits` is the number of correctly classified rows of that batch (0-dim int64 tensor on the
    logits' device, no host read) and `last_count` the batch size, so the training accuracy costs no second pass
    (Modules/train_rnn_quake.py reads both with the loss in one transfer). y: B or B x 1, int64 or a floating tensor of integers.
    CPU tensors (the gloo tests run the harness on CPU) and logits the kernel does not take (C > 1024, other dtypes, not 2-D) go
    through torch's own expressions; non-contiguous logits are made contiguous."""

    def __init__(self):
        self.last_hits, self.last_count = None, 0

    def __call__(self, yHat, y):
        from .. import ops
        B = yHat.shape[0]
        lab = _labels(y, B)
        self.last_count = B
        if yHat.is_cuda and yHat.dim() == 2 and lab.dim() == 1:
            loss, self.last_hits = ops.cross_entropy(yHat, lab, return_hits=True)
            return loss
        loss = torch.nn.functional.cross_entropy(yHat, lab)
        self.last_hits = (torch.argmax(yHat.detach(), dim=1) == lab).sum()
        return loss


crossEntropyLoss = CrossEntropyLoss()          # one shared instance, as the driver shares one nn.CrossEntropyLoss() among its models


def accuracy(yHat, y, tol=1e-9):
    """Ratio of rows with argmax(yHat) == y (reference QuakeData.evaluate, dataTools.py:1564-1586; `tol` is the reference's threshold
    on |argmax - y|, which for integer labels is equality). Device logits [B][C]: ops.accuracy (the cross-entropy kernel without a
    gradient), a 0-dim device tensor in fp64 for fp64 logits, else fp32; anything else: the torch expression."""
    B = yHat.shape[0]
    if yHat.is_cuda and yHat.dim() == 2 and y.numel() == B:
        from .. import ops
        return ops.accuracy(yHat, y)
    out_dt = torch.float64 if yHat.dtype == torch.float64 else torch.float32
    pred = torch.argmax(yHat, dim=1).to(torch.float64)
    errors = torch.sum(torch.abs(pred - y.reshape(pred.shape).to(torch.float64)) > tol)
    return 1 - errors.to(out_dt) / B
