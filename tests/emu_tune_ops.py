"""TEST INFRASTRUCTURE: tests/emu_train_ops.py (the fp32 torch-CPU emulation of ``motioneditor_amd.ops`` with the derived-weight refresh) plus what the widened
stage-1 tuner adds to that interface: ``groupnorm_bwd(dgamma=, dbeta=)`` (include/motioned_tune.h me_groupnorm_bwd_params) and the folded-upsampler entries of
``refresh_table`` / ``refresh_weights`` (me_refresh_ups4).  Neither is restated by hand: the affine gradients are torch autograd of the forward emulation, the
fold is weights.Packed.fold_ups.  ``gemm_dw(conv=...)`` needs nothing new here: emu_ops.gemm_dw differentiates every gather of its forward."""
from __future__ import annotations

import torch

import emu_train_ops
from emu_train_ops import *  # noqa: F401,F403

globals().update({k: v for k, v in vars(emu_train_ops).items() if k.startswith("_") and not k.startswith("__")})


def groupnorm_bwd(x, gamma, beta, dy, *, rows_per_group, eps, silu, groups=32, dgamma=None, dbeta=None):
    """dx; dgamma / dbeta (fp32 [C], either may be None) are ACCUMULATED into."""
    x0, g0, b0 = _leaf(x), _leaf(gamma), _leaf(beta)   # noqa: F405
    y = groupnorm(x0, g0, b0, rows_per_group=rows_per_group, eps=eps, silu=silu, groups=groups)   # noqa: F405
    dx, dg, db = torch.autograd.grad(y, [x0, g0, b0], dy.float())
    if dgamma is not None:
        dgamma.add_(dg)
    if dbeta is not None:
        dbeta.add_(db)
    return dx


def fold_ups_packed(master: torch.Tensor) -> torch.Tensor:
    """fp32 [N, 9, K] (tap-major packing) -> Packed.fold_ups of the same weight, fp32 [N, 16, K] (unrounded)."""
    from motioneditor_amd.weights import Packed
    n, taps, k = master.shape
    assert taps == 9
    return Packed.fold_ups(master.reshape(n, 3, 3, k).permute(0, 3, 1, 2).contiguous())


def refresh_table(entries):
    return list(entries)


def refresh_weights(table) -> None:
    plain = [e for e in table if e[0].dim() != 3]
    emu_train_ops.refresh_weights(plain)
    for m, d, *_ in table:
        if m.dim() == 3:     # a folded upsampler weight: the fp32 sums rounded once to dst's dtype
            d.copy_(fold_ups_packed(m.float().cpu()).to(d.dtype))
