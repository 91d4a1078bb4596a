"""Loss seeds of the training step as ONE launch each (forward + gradient), with the constructor surface of the reference.

* `FocalLoss` mirrors `losses/focal_loss.py:15-118` -- same arguments, same defaults, and the behaviour the class actually
  has: the live `_process_preds` (84-91) clamps to [eps, 1-eps] and softmaxes, and `forward` (92-110) calls it twice.
* `CrossEntropyLoss` is the `train.py:178-179` alternative (torch.nn.CrossEntropyLoss, mean reduction, ignore_index -100).
* `StepMeter` replaces the two per-step host reads of `train.py:327-328` (`running_loss += loss.item() * B`,
  `num_acc += (argmax == labels).sum().item()`): the loss kernel accumulates both on the device; read once per epoch.

* A `data.MixedTarget` (Mixup / CutMix, `data.BatchMix`) as `target`, or `CrossEntropyLoss(label_smoothing=e)`, takes the second kernel of
  the same file: row i costs lam_i l(x_i, a_i) + (1 - lam_i) l(x_i, b_i) in ONE launch -- timm's Mixup + SoftTargetCrossEntropy without the
  dense target matrix, with per-sample lam, class weights, ignored rows and the meter counted once.

* Labels are checked on the device.  A label that is neither `ignore_index` nor a class in [0, K) -- a label file numbered 1..K, say --
  cannot raise as torch does (the step makes no host read), so it is answered with NaN: that row's loss and gradient row are NaN, the
  'mean' / 'sum' loss is NaN, and the meter does not count the row as correct.  A batch whose rows are all ignored has a NaN 'mean' loss;
  `CrossEntropyLoss` then returns all-zero gradients as torch does, `FocalLoss` NaN gradients as its reference does (0 at the logits
  its clamp cuts off).

The kernels live in `csrc/loss.hip` (`gvk_loss_fwd_bwd`, `gvk_loss_mixed_fwd_bwd`); there is no torch fallback.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor, nn

from . import ops
from .data import MixedTarget


class StepMeter:
    """Device-side running sums of an epoch: loss * batch, correct argmax predictions, samples.

    buf[0] gains, per step of B samples: 'mean' -> the reduced loss * B (train.py:327); 'sum' -> the summed loss * B, as train.py's
    formula does with whatever the criterion returns; 'none' -> the sum of the B per-sample losses, i.e. what 'mean' adds for an
    unweighted batch with no ignored rows.  read() divides by the samples seen, so under 'mean' and 'none' it gives the mean loss."""

    def __init__(self, device):
        self.buf = torch.zeros(3, dtype=torch.float32, device=device)

    def reset(self) -> None:
        self.buf.zero_()

    def read(self):
        """(mean loss, accuracy, samples) -- the one host read (train.py:330-331 do this division per epoch)."""
        loss_sum, correct, n = self.buf.tolist()
        n = max(n, 1.0)
        return loss_sum / n, correct / n, int(n)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, mod):
        x = logits.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        none = mod.reduction == "none"
        loss = torch.empty(x.shape[0] if none else 1, dtype=torch.float32, device=x.device)
        dlogits = torch.empty_like(x)
        kw = dict(gamma=float(mod._gamma), eps=float(mod.eps), ignore_index=int(mod.ignore_index), weights=mod._weights_on(x.device),
                  meter=mod.meter.buf if mod.meter is not None else None, reduction=mod.reduction)
        if isinstance(target, MixedTarget):
            ops.loss_mixed_fwd_bwd(x, target.a.contiguous().view(-1), target.b.contiguous().view(-1), target.lam.float().contiguous().view(-1),
                                   loss, dlogits, mod._kind, smoothing=float(mod.label_smoothing), **kw)
        elif mod.label_smoothing > 0:                    # plain label smoothing: no partner
            ops.loss_mixed_fwd_bwd(x, target.contiguous().view(-1), None, None, loss, dlogits, mod._kind, smoothing=float(mod.label_smoothing), **kw)
        else:
            ops.loss_fwd_bwd(x, target.contiguous().view(-1), loss, dlogits, mod._kind, **kw)
        ctx.save_for_backward(dlogits)
        ctx.in_dtype = logits.dtype
        ctx.none = none
        return loss if none else loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (dlogits,) = ctx.saved_tensors
        if ctx.none:                                     # reduction='none': row i of dlogits is d loss_i / d logits_i
            return (dlogits * grad_out.reshape(-1, 1)).to(ctx.in_dtype), None, None
        return (dlogits * grad_out).to(ctx.in_dtype), None, None


class _FusedLoss(nn.Module):
    _kind = ops.LOSS_CE
    _gamma = 0.0
    eps = 1e-16
    ignore_index = -100
    reduction = "mean"
    label_smoothing = 0.0
    weights: Optional[Tensor] = None
    meter: Optional[StepMeter] = None

    def attach_meter(self, meter: Optional[StepMeter]):
        self.meter = meter
        return self

    def _weights_on(self, device):
        if self.weights is None:
            return None
        if self.weights.device != device or self.weights.dtype != torch.float32:
            self.weights = self.weights.to(device=device, dtype=torch.float32).contiguous()
        return self.weights

    def forward(self, x: Tensor, target: Union[Tensor, MixedTarget]) -> Tensor:
        if x.dim() != 2 or x.shape[-1] < 2:
            raise NotImplementedError("the fused loss takes [batch, classes >= 2] logits (train.py feeds [B, num_classes])")
        if isinstance(target, Tensor) and target.is_floating_point():
            raise NotImplementedError("dense [B][K] probability targets are not built: pass class indices, or the pair data.MixedTarget(a, b, lam)")
        return _LossFn.apply(x, target, self)


class FocalLoss(_FusedLoss):
    _kind = ops.LOSS_FOCAL

    def __init__(self, gamma, weights: Union[None, Tensor] = None, reduction: str = "mean", ignore_index=-100, eps=1e-16, fp16: bool = False) -> None:
        super().__init__()
        if reduction not in ["mean", "none", "sum"]:
            raise NotImplementedError("Reduction {} not implemented.".format(reduction))
        assert weights is None or isinstance(weights, Tensor), "weights should be of type Tensor or None, but {} given".format(type(weights))
        self.dtype = torch.float16 if fp16 else torch.float32
        self.reduction = reduction
        self.gamma = gamma
        self._gamma = gamma
        self.ignore_index = ignore_index
        self.eps = eps
        self.weights = weights


class CrossEntropyLoss(_FusedLoss):
    _kind = ops.LOSS_CE

    def __init__(self, weight: Optional[Tensor] = None, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0) -> None:
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise NotImplementedError("Reduction {} not implemented.".format(reduction))
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError("label_smoothing must be between 0.0 and 1.0. Got: {}".format(label_smoothing))
        self.label_smoothing = float(label_smoothing)
        self.weights = weight
        self.ignore_index = ignore_index
        self.reduction = reduction
