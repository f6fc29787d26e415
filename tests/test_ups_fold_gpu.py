"""me_gemm gather mode ups = 3 on a real MI355X: the 3x3 convolution over a nearest-2x upsample run as four 2x2-tap convolutions on pre-summed weights.

Reference: the fp64 convolution of the upsampled input on the CPU (tests/ups_fold_ref.py).  e1 = rel-L2 of the EXISTING ups = 1 launch against that
reference with the original weights, same terms.  Bounds:
  kernel      ups = 3 against the fp64 reference computed with the ROUNDED FOLDED weights   <= 1.25 e1        (same arithmetic, another summation order)
  end to end  ups = 3 against the reference with the original weights                        <= 1.25 e1 + d    (d = rel-L2 between the two fp64 references)
The original weights are fp16 values (what ups = 1 multiplies), so e1 is the launch's own arithmetic error and nothing else.
Every figure is printed before it is asserted."""
import fnmatch

import numpy as np
import pytest
import torch

from conftest import GOLD, rel_l2 as rel_l2_conftest
from guard import embed_in, run_guarded, sentinel_out
from ups_fold_ref import conv_fold_ref, conv_ups_ref, rel_l2

from motioneditor_amd.weights import Packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


# (Cin, Cout, H, W, n_img, forced kernel or None): the smallest shapes at which each path can go wrong
SHAPES = {
    "1x1 all taps but one in padding": (64, 64, 1, 1, 3, None),
    "5x7 odd, ragged 128-row tile": (64, 128, 5, 7, 2, None),
    "640 4x4 (test_gemm_conv3x3's case)": (640, 640, 4, 4, 3, None),
    "8p 256-row": (64, 320, 8, 8, 8, "256"),
    "8p 192-row": (64, 320, 8, 8, 8, "192"),
    "vae 512": (512, 512, 8, 8, 1, None),
    "vae 256": (256, 256, 8, 8, 2, None),
    "K tail 72 (global_load_lds staging)": (72, 64, 3, 5, 2, None),      # K % 64 != 0 takes the other staging path
}
TERMS = ["bias", "bias+rowvec", "bias+res in place", "ldc = N + 320"]


def force(monkeypatch, which):
    """Per-call dispatch switches: put a small launch on one of the two 8-phase gather kernels (tiles then span images; four parities of row tiles)."""
    for k in ("ME_GEMM_8P", "ME_GEMM_ROWEPI", "ME_GEMM_BUF"):
        monkeypatch.delenv(k, raising=False)
    if which == "256":
        monkeypatch.setenv("ME_GEMM_BIG_MIN", "1")
    elif which == "192":
        monkeypatch.setenv("ME_GEMM_BIG_MIN", str(1 << 40))
        monkeypatch.setenv("ME_GEMM_8P_192", "1")
        monkeypatch.setenv("ME_GEMM_192_MINK", "1")
    else:
        for k in ("ME_GEMM_BIG_MIN", "ME_GEMM_8P_192", "ME_GEMM_192_MINK"):
            monkeypatch.delenv(k, raising=False)


def want_kernel(which):
    return {"256": "gemm8p_kernel<256,320,true>", "192": "gemm8p_kernel<192,320,true>", None: "gemm_kernel<128,*>"}[which]


_REFS = {}


def problem(shape):
    """Inputs and the two term-free fp64 references of a shape, computed once and shared (never modified)."""
    if shape not in _REFS:
        Cin, Cout, H, W, n_img, _ = SHAPES[shape]
        x = rnd(n_img * H * W, Cin, seed=1)
        w4 = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5).float()        # fp16 values: the original weights are what ups = 1 multiplies
        w9 = Packed._as_taps(w4).contiguous().half()
        w16 = Packed({"w": w4}, "cpu").mat_ups("w")                                 # fp32 sums, one rounding
        assert torch.equal(w9.float(), Packed._as_taps(w4)) and w16.shape == (Cout, 16, Cin)
        M = n_img * 4 * H * W
        d = dict(x=x, w9=w9, w16=w16, M=M, bias=rnd(Cout, seed=3), rowvec=rnd(n_img, Cout, seed=4), res=rnd(M, Cout, seed=5),
                 ref_orig=conv_ups_ref(x, w9, n_img, H, W), ref_fold=conv_fold_ref(x, w16, n_img, H, W))
        d["delta"] = rel_l2(d["ref_fold"], d["ref_orig"])
        _REFS[shape] = d
    return _REFS[shape]


def launch(ops, p, shape, terms, ups):
    Cin, Cout, H, W, n_img, _ = SHAPES[shape]
    conv = (H, W, 2 * H, 2 * W, 1, ups)
    w = (p["w16"] if ups == 3 else p["w9"]).cuda()
    kw = dict(M=p["M"], bias=p["bias"].cuda(), conv=conv)
    if terms == "bias+rowvec":            # one vector row per image: a tile holds rows of several images
        kw.update(rowvec=p["rowvec"].cuda(), rows_per_vec=4 * H * W)
    if terms == "bias+res in place":
        buf = p["res"].cuda().clone()
        out = ops.gemm(p["x"].cuda(), w, res=buf, out=buf, **kw)
        assert out.data_ptr() == buf.data_ptr()
        return out
    if terms == "ldc = N + 320":          # the left columns of a wider buffer (the up path's concat buffer)
        wide = torch.full((p["M"], Cout + 320), 7.0, dtype=torch.float16, device="cuda")
        out = ops.gemm(p["x"].cuda(), w, out=wide[:, :Cout], **kw)
        assert bool((wide[:, Cout:] == 7.0).all()), "columns [N, ldc) were written"
        return out
    return ops.gemm(p["x"].cuda(), w, **kw)


def with_terms(p, shape, terms, ref):
    Cin, Cout, H, W, n_img, _ = SHAPES[shape]
    y = ref + p["bias"].double()[None]
    if terms == "bias+rowvec":
        y = y + p["rowvec"].double().repeat_interleave(4 * H * W, dim=0)
    if terms == "bias+res in place":
        y = y + p["res"].double()
    return y


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ups3_kernel_and_end_to_end_error(ops, shape, terms, monkeypatch):
    p = problem(shape)
    which = SHAPES[shape][5]
    force(monkeypatch, which)
    y1 = launch(ops, p, shape, terms, 1)
    k1 = ops._last_kernel()
    y3 = launch(ops, p, shape, terms, 3)
    k3 = ops._last_kernel()
    assert torch.isfinite(y3.float()).all()
    ref_orig, ref_fold = with_terms(p, shape, terms, p["ref_orig"]), with_terms(p, shape, terms, p["ref_fold"])
    e1 = rel_l2(y1, ref_orig)
    ek, ee = rel_l2(y3, ref_fold), rel_l2(y3, ref_orig)
    print(f"{shape} [{terms}]: e1 {e1:.3e} ({k1}); ups3 vs folded reference {ek:.3e} (<= {1.25 * e1:.3e}); vs original {ee:.3e} "
          f"(<= {1.25 * e1 + p['delta']:.3e}, delta {p['delta']:.3e}) ({k3})")
    assert fnmatch.fnmatchcase(k3, want_kernel(which)) and fnmatch.fnmatchcase(k1, want_kernel(which)), (k1, k3)
    assert ek <= 1.25 * e1, f"kernel: {ek:.3e} > 1.25 x {e1:.3e}"
    assert ee <= 1.25 * e1 + p["delta"], f"end to end: {ee:.3e} > 1.25 x {e1:.3e} + {p['delta']:.3e}"


@pytest.mark.parametrize("shape", ["5x7 odd, ragged 128-row tile", "8p 256-row", "8p 192-row"])
def test_ups3_stays_inside_its_views(ops, shape, monkeypatch):
    """Guard band: the output lies between sentinel rows and sentinel columns (ldc > N), the inputs in poison; three launches on NaN / 0 / 6e4 surroundings
    give the same finite bits and leave every sentinel untouched (guard.run_guarded)."""
    p = problem(shape)
    Cin, Cout, H, W, n_img, which = SHAPES[shape]
    force(monkeypatch, which)
    ins = {"x": embed_in(p["x"], device="cuda"), "w": embed_in(p["w16"], device="cuda", contiguous=True, row_guard=320 * 16, col_guard=Cin),
           "bias": embed_in(p["bias"], device="cuda", contiguous=True)}
    out, _ = sentinel_out((p["M"], Cout), device="cuda")
    assert out.stride(0) > Cout
    got = run_guarded(lambda: ops.gemm(ins["x"], ins["w"], M=p["M"], bias=ins["bias"], conv=(H, W, 2 * H, 2 * W, 1, 3), out=out), ins, {"out": out})["out"]
    assert fnmatch.fnmatchcase(ops._last_kernel(), want_kernel(which)), ops._last_kernel()
    e = rel_l2(got, with_terms(p, shape, "bias", p["ref_fold"]))
    print(f"{shape}: guarded launch {e:.3e} from the folded reference")
    assert e <= 2e-3      # (the suite's kernel bound, tests/guard.py REL_L2: the tight bound is the error test's)


@pytest.mark.parametrize("which", [None, "256", "192"])
def test_ups3_sub_batch_is_bitwise_the_rows_of_the_full_launch(ops, which, monkeypatch):
    """sel_rows: two images computed alone, with the kernel selected as for four, are bitwise the first half of the four-image launch."""
    Cin, Cout, H, W = (64, 320, 8, 8) if which else (64, 128, 5, 7)
    force(monkeypatch, which)
    x = rnd(4 * H * W, Cin, seed=11).cuda()
    w16 = Packed({"w": rnd(Cout, Cin, 3, 3, seed=12, scale=(9 * Cin) ** -0.5).float()}, "cuda").mat_ups("w")
    bias = rnd(Cout, seed=13).cuda()
    conv = (H, W, 2 * H, 2 * W, 1, 3)
    full = ops.gemm(x, w16, M=4 * 4 * H * W, bias=bias, conv=conv)
    k_full = ops._last_kernel()
    monkeypatch.setattr(ops, "SELECT_ROWS_SCALE", 2)
    half = ops.gemm(x[:2 * H * W], w16, M=2 * 4 * H * W, bias=bias, conv=conv)
    assert ops._last_kernel() == k_full and fnmatch.fnmatchcase(k_full, want_kernel(which)), (ops._last_kernel(), k_full)
    assert torch.equal(half, full[:2 * 4 * H * W]), f"{int((half != full[:2 * 4 * H * W]).sum())} elements differ"


def test_ups3_rejects_what_it_does_not_cover(ops):
    x, w = rnd(16, 64).cuda(), rnd(64, 16, 64).cuda()
    from motioneditor_amd import capi
    with pytest.raises(Exception):
        ops.gemm(x, w, M=64, conv=(4, 4, 8, 8, 2, 3))          # stride 2
    with pytest.raises(Exception):
        ops.gemm(x, w, M=64, conv=(4, 4, 8, 7, 1, 3))          # Wout != 2 Win
    with pytest.raises(ValueError):
        ops.gemm(x, rnd(64, 9, 64).cuda(), M=64, conv=(4, 4, 8, 8, 1, 3))   # nine taps
    assert capi.lib().me_abi_version() == 9


@pytest.mark.parametrize("tag,step", [("inactive", 0)])
def test_two_branch_unet_fold_on_and_off_vs_golden(unet_sd_np, tag, step, monkeypatch):
    """The smallest two-branch golden (batch 4, 16 frames, 16 x 16 latents, tests/test_model_gpu.py): the forward with the fold on and off both meet the
    golden's tolerance, and the two runs lie closer to each other than the fold-off run lies to the golden."""
    from motioneditor_amd import synth
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from test_model_gpu import UNET_TOL, editors
    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    g = torch.from_numpy(np.load(GOLD / f"unet_two_{tag}.npz")["out"])
    c = synth.make_case_inputs("two", B=4, f=16, h=16, w=16)
    outs = {}
    for fold in ("0", "1"):
        monkeypatch.setenv("ME_UPS_FOLD", fold)
        sed, ted = editors(unet, c["source_masks"])
        sed.cur_step = ted.cur_step = step
        outs[fold] = unet(c["sample"].cuda(), c["t"], c["ehs"].cuda(), down_block_additional_residuals=[d.cuda() for d in c["down_res"]],
                          mid_block_additional_residual=c["mid_res"].cuda()).sample.float().cpu()
        unet.spatial_editor = unet.temporal_editor = None
    has_fold = any(k.startswith("ups4:") for k in unet.P.cache)
    e_off, e_on, d = rel_l2_conftest(outs["0"], g), rel_l2_conftest(outs["1"], g), rel_l2_conftest(outs["1"], outs["0"])
    print(f"two-branch UNet vs golden: fold off {e_off:.4e}, fold on {e_on:.4e} (<= {UNET_TOL}); on vs off {d:.4e}")
    assert has_fold, "the forward with ME_UPS_FOLD=1 packed no folded weight"
    assert e_off <= UNET_TOL and e_on <= UNET_TOL
    assert 0.0 < d < e_off
