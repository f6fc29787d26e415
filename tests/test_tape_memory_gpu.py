"""The memory-lean, checkpointing autodiff tape on a real MI355X.  8 frames on 8 x 8 latents: the three forms of the tape
(tests/tape_memory_common.py) give bitwise the same adapter gradients, null-text gradient / embedding and tuned masters on the HIP kernels, with the
recomputation check on.  72 frames on 8 x 8 latents (two key stages, two query blocks, nine adapter chunks, the key-tiled backward pair -- the shape
test_long_bwd_gpu.py pins against the oracle in lean form): checkpointed == lean, bitwise.  16 frames on 16 x 16 latents: the allocator's peak of one
adapter step orders checkpointed < lean < parent.  examples/train_adapter.py prints the same losses with and without --gradient-checkpointing."""
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import bwd_run as br
import tape_memory_common as tm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def unet(unet_sd_np):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi
    capi.lib()  # fails loudly when libmotioned.so is missing
    return tm.make_unet(unet_sd_np, "cuda")


def _same_grads(a, b):
    return sorted(a) == sorted(b) and [k for k in a if not tm.same(a[k], b[k])] == []


def test_adapter_gradients_are_bitwise_the_same_in_all_three_forms(unet):
    l0, g0, s0 = tm.adapter_grads(unet, "parent")
    assert len(g0) > 300 and any(float(g.abs().max()) > 0 for g in g0.values())
    seen = {"parent": s0}
    for name in ("lean", "ckpt"):
        l, g, seen[name] = tm.adapter_grads(unet, name)
        assert l == l0 and _same_grads(g, g0), name
    print(seen)
    assert seen["ckpt"]["stashed_bytes"] < seen["lean"]["stashed_bytes"] < seen["parent"]["stashed_bytes"]
    assert seen["lean"]["grad_peak_bytes"] < seen["parent"]["grad_total_bytes"] == seen["parent"]["grad_peak_bytes"]


def test_null_text_gradient_and_embedding_are_bitwise_the_same_in_all_three_forms(unet):
    g0, e0 = tm.null_text(unet, "parent")
    assert float(g0.abs().max()) > 0
    for name in ("lean", "ckpt"):
        g, e = tm.null_text(unet, name)
        assert tm.same(g, g0) and tm.same(e, e0), name


@pytest.mark.parametrize("which", sorted(tm.TUNER_SETS))
def test_unet_tuner_step_ends_with_bitwise_the_parent_forms_masters(unet_sd_np, unet, which):
    l0, m0 = tm.tuner_masters(unet_sd_np, "cuda", "parent", which)
    for name in ("lean", "ckpt"):
        l, m = tm.tuner_masters(unet_sd_np, "cuda", name, which)
        assert l == l0 and tm.same(m, m0), (which, name)


def test_72_frames_checkpointed_is_bitwise_the_lean_form(unet):
    l0, g0, _ = tm.adapter_grads(unet, "lean", f=72)
    l1, g1, _ = tm.adapter_grads(unet, "ckpt", f=72)
    assert l1 == l0 and _same_grads(g1, g0)
    n0, _ = tm.null_text(unet, "lean", f=72, inner=1)
    n1, _ = tm.null_text(unet, "ckpt", f=72, inner=1)
    assert float(n0.abs().max()) > 0 and tm.same(n1, n0)


def test_peak_memory_of_an_adapter_step_orders_checkpointed_lean_parent(unet):
    """16 frames on 16 x 16 latents.  Each form: a warm-up step, empty_cache() + reset_peak_memory_stats(), one step, max_memory_allocated().  Only the
    ordering is asserted."""
    from motioneditor_amd import util
    c = br.training_clip(0, f=16, h=16)
    c = {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}
    peak = {}
    for name in tm.FORMS:
        with tm.form(name) as ckpt:
            for warm in (True, False):
                loss, grads = util.adapter_training_grads(unet, c["noisy"], c["t"], c["ehs"], c["down"], c["mid"], c["noise"], gradient_checkpointing=ckpt)
                del grads
                if warm:
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated()
    print({k: f"{v / 2 ** 20:.1f} MiB" for k, v in peak.items()})
    assert peak["ckpt"] < peak["lean"] < peak["parent"], peak


def test_example_prints_the_same_losses_with_gradient_checkpointing():
    def run(*extra):
        r = subprocess.run([sys.executable, str(ROOT / "examples" / "train_adapter.py"), "--frames", "72", "--size", "128", *extra],
                           capture_output=True, text=True, timeout=300, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        losses = re.findall(r"loss = ([0-9.eE+-]+|nan|inf)", r.stdout)
        assert len(losses) == 2, r.stdout
        return losses
    plain, ckpt = run(), run("--gradient-checkpointing")
    print(plain, ckpt)
    assert plain == ckpt and all(float(x) == float(x) for x in plain)
