"""TEST INFRASTRUCTURE: tests/emu_ops.py (the fp32 torch-CPU emulation of every ``motioneditor_amd.ops`` entry point) plus the derived-weight
refresh of the stage-1 UNet tuner (ops.refresh_table / ops.refresh_weights, csrc/train.hip me_refresh_weights).  Tests assign this module as
``ops`` where the tuner runs."""
from __future__ import annotations

import emu_ops
from emu_ops import *  # noqa: F401,F403

globals().update({k: v for k, v in vars(emu_ops).items() if k.startswith("_") and not k.startswith("__")})


def refresh_table(entries):
    return list(entries)


def refresh_weights(table) -> None:
    """plain entry: dst = master (in dst's dtype); fold entry: dst = (master * gamma) rounded to dst's dtype, colsum = row sums of the ROUNDED dst,
    cvec = master @ beta (+ bias) -- weights.Packed.ln_fold from the same values."""
    for m, d, gamma, beta, bias, colsum, cvec in table:
        if gamma is None:
            d.copy_(m.to(d.dtype))
            continue
        wq = (m * gamma[None, :]).to(d.dtype)
        d.copy_(wq)
        colsum.copy_(wq.float().sum(dim=1))
        cv = m @ beta
        cvec.copy_(cv + bias if bias is not None else cv)
