"""Stage-1 tuning widened to the 3x3 convolutions and the GroupNorm affine parameters, without a GPU: util.UNetTuner on the emulated ABI (tests/emu_tune_ops.py)
against oracle.ref_cpu.unet_forward under torch autograd + clip_grad_norm_ + torch.optim.AdamW, the layouts of what it exports, the names it still refuses,
the ABI table of include/motioned_tune.h (capi.TUNE_SYMBOLS) with the guard rule of tests/test_clip_io_cpu.py, and the argument contract of its three
launching entries.  Bounds: those of tests/test_bg_train_cpu.py."""
import ctypes
import re

import pytest
import torch

import emu_tune_ops
import tune_fixture as tf
from conftest import ROOT


@pytest.fixture
def emu(monkeypatch):
    import motioneditor_amd.models.unet_2d_condition as u
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    for m in (graph, u, util):
        monkeypatch.setattr(m, "ops", emu_tune_ops)


def _unet(sd_np):
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    return UNet2DConditionModel(sd_np, device="cpu", dtype=torch.float32)


# ------------------------------------------------------------------ the emulation itself
def test_emulated_groupnorm_params_and_ups4_refresh_are_autograd_and_fold_ups():
    """dgamma / dbeta accumulate (+=) the autograd gradients of the forward emulation next to an unchanged dx; a folded-upsampler refresh entry is
    Packed.fold_ups of the master rounded once; plain entries still go through emu_train_ops."""
    import emu_ops
    from motioneditor_amd.weights import Packed
    g = torch.Generator().manual_seed(3)
    x, gm, bt, dy = torch.randn(24, 64, generator=g), 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g), torch.randn(24, 64, generator=g)
    for silu in (False, True):
        dg0, db0 = torch.randn(64, generator=g), torch.randn(64, generator=g)
        dg, db = dg0.clone(), db0.clone()
        dx = emu_tune_ops.groupnorm_bwd(x, gm, bt, dy, rows_per_group=12, eps=1e-5, silu=silu, dgamma=dg, dbeta=db)
        assert torch.equal(dx, emu_ops.groupnorm_bwd(x, gm, bt, dy, rows_per_group=12, eps=1e-5, silu=silu))
        gl, bl = gm.clone().requires_grad_(True), bt.clone().requires_grad_(True)
        wg, wb = torch.autograd.grad(emu_ops.groupnorm(x, gl, bl, rows_per_group=12, eps=1e-5, silu=silu), [gl, bl], dy)
        assert torch.allclose(dg - dg0, wg, rtol=1e-5, atol=1e-5) and torch.allclose(db - db0, wb, rtol=1e-5, atol=1e-5)
        only = torch.zeros(64)
        emu_tune_ops.groupnorm_bwd(x, gm, bt, dy, rows_per_group=12, eps=1e-5, silu=silu, dbeta=only)     # either output may be missing
        assert torch.allclose(only, wb, rtol=1e-5, atol=1e-5)
    w = torch.randn(8, 16, 3, 3, generator=g)
    master = Packed._as_taps(w).contiguous()
    dst16, plain = torch.zeros(8, 16, 16, dtype=torch.float16), torch.zeros(8, 9 * 16, dtype=torch.float16)
    emu_tune_ops.refresh_weights(emu_tune_ops.refresh_table([(master, dst16, None, None, None, None, None), (master.reshape(8, -1), plain, None, None, None, None, None)]))
    assert torch.equal(dst16, Packed.fold_ups(w).half()) and torch.equal(plain, master.reshape(8, -1).half())


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("C,groups,rpg,nsg", tf.GN_CASES)
def test_emulated_groupnorm_params_meet_the_layernorm_params_bounds_against_fp64(C, groups, rpg, nsg, silu):
    """The GPU test holds me_groupnorm_bwd_params to BOUNDS["layernorm_bwd_params.dgamma" / ".dbeta"] on these inputs: the fp32 emulation meets them against the
    fp64 reference here, so the bounds are reachable by fp32 accumulation and the entry needs none of its own."""
    from bwd_cases import BOUNDS
    from guard import errs
    x, gamma, beta, dy, g0, b0 = tf.gn_inputs(C, rpg, nsg)
    dg, db = torch.zeros(C), torch.zeros(C)
    emu_tune_ops.groupnorm_bwd(x, gamma, beta, dy, rows_per_group=rpg, eps=1e-5, silu=silu, groups=groups, dgamma=dg, dbeta=db)
    wg, wb = tf.gn_params_ref64(x, gamma, beta, dy, rpg, groups, silu)
    for nm, got, want in (("dgamma", dg, wg), ("dbeta", db, wb)):
        r, m = errs(got, want)
        print(f"emulated groupnorm_bwd params {nm} C={C} rpg={rpg} silu={silu}: rel-L2 {r:.3e}, max/mean {m:.3e}")
        assert r <= BOUNDS["layernorm_bwd_params." + nm][0] and m <= BOUNDS["layernorm_bwd_params." + nm][1], (nm, r, m)


@pytest.mark.parametrize("n_img,Hin,Win,stride,ups", [(2, 5, 7, 1, 0), (3, 1, 1, 1, 0), (2, 7, 9, 2, 0), (2, 3, 5, 1, 1)])
def test_emulated_conv_dw_meets_the_gemm_dw_bound_against_fp64(n_img, Hin, Win, stride, ups):
    """The shapes of the GPU test (N 40, K 72): emu_ops.gemm_dw(conv=...) against ref64_bwd.gemm_dw(conv=...) inside BOUNDS["gemm_dw"]."""
    from bwd_cases import BOUNDS
    from guard import errs
    x, dy, dst0, conv, M = tf.conv_dw_inputs(n_img, Hin, Win, 40, 72, stride, ups)
    got = emu_tune_ops.gemm_dw(dy.half().float(), x, dst=dst0.clone(), taps=9, K=72, M=M, alpha=0.5, conv=conv)
    r, m = errs(got.double() - dst0.double(), tf.conv_dw_ref64(x, dy, conv, M, 0.5))
    assert r <= BOUNDS["gemm_dw"][0] and m <= BOUNDS["gemm_dw"][1], (r, m)


# ------------------------------------------------------------------ the tuner on the emulated ABI
def test_the_widened_selection_covers_every_accepted_kind(unet_sd_np):
    names = tf.selected(unet_sd_np)
    for frag in ("resnets.0.conv1.weight", "resnets.1.conv2.bias", "conv_shortcut.weight", "downsamplers.0.conv.weight", "upsamplers.0.conv.bias", "proj_in.weight",
                 "proj_out.bias", "resnets.2.norm1.weight", "resnets.0.norm2.bias", "attentions.0.norm.weight", "attn1.to_q.weight", "attn_temp.to_out.0.bias"):
        assert any(n.endswith(frag) for n in names), frag
    assert not any("temp_conv" in n or "time_emb" in n or "transformer_blocks.0.norm" in n or n.startswith(("conv_in", "conv_out")) for n in names)


def test_tuner_gradients_of_convolutions_and_groupnorms_match_autograd(emu, unet_sd_np):
    """UNetTuner.grads at the widened selection against the oracle's autograd gradients: per-parameter rel-L2 < 2e-3, loss to 1e-4 relative; every gradient in
    the shape of its parameter.  (At 1 x 1 pixel -- mid block, down_blocks.3 -- only the centre tap of a 3x3 weight has a gradient: checked explicitly.)"""
    from motioneditor_amd import util
    o, c = tf.oracle(), tf.golden()
    tr = util.UNetTuner(_unet(unet_sd_np), trainable_modules=tf.MODULES)
    assert tr.names == o["names"]
    loss, grads = tr.grads(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert abs(loss - o["losses"][0]) < 1e-4 * o["losses"][0], (loss, o["losses"][0])
    errs = {}
    for k in tr.names:
        assert grads[k].shape == o["grads"][k].shape == torch.Size(unet_sd_np[k].shape), k
        errs[k] = float((grads[k] - o["grads"][k]).norm() / o["grads"][k].norm())
    worst = max(errs, key=errs.get)
    print(f"widened stage-1 gradients on the emulated ABI: {len(errs)} parameters, worst rel-L2 {errs[worst]:.3e} ({worst})")
    assert errs[worst] < 2e-3, (worst, errs[worst])
    g1 = grads["mid_block.resnets.0.conv1.weight"]
    assert float(g1[:, :, 1, 1].abs().max()) > 0 and float(g1.abs().sum() - g1[:, :, 1, 1].abs().sum()) == 0.0


def test_tuner_steps_match_autograd_adamw_and_leave_everything_else_bitwise(emu, unet_sd_np):
    """Two tuner steps against two oracle steps; every parameter outside the bucket -- temporal convolutions, time_emb_proj, LayerNorms, conv_in / conv_out, the
    frozen k|v rows, the adapter -- bitwise unchanged, in the state and in the packed tensors the forward reads."""
    from motioneditor_amd import util
    from motioneditor_amd.weights import Packed
    o, c = tf.oracle(), tf.golden()
    unet = _unet(unet_sd_np)
    tr = util.UNetTuner(unet, trainable_modules=tf.MODULES, lr=tf.LR)
    l1 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    l2 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got, want, sd = tr.export_state_dict(), o["after"][1], o["sd"]
    assert abs(l1 - o["losses"][0]) < 1e-4 * o["losses"][0] and abs(l2 - o["losses"][1]) < 1e-4 * o["losses"][1], (l1, l2, o["losses"])
    num = sum(float((got[k] - want[k]).pow(2).sum()) for k in tr.names)
    den = sum(float((want[k] - sd[k]).pow(2).sum()) for k in tr.names)
    print("two widened steps on the emulated ABI: update rel-L2", (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5
    for kind in (".conv1.weight", ".norm1.weight", "upsamplers.0.conv.weight", "proj_in.bias"):     # each new kind moved, and towards the oracle
        ks = [k for k in tr.names if k.endswith(kind)]
        n_k = sum(float((got[k] - want[k]).pow(2).sum()) for k in ks)
        d_k = sum(float((want[k] - sd[k]).pow(2).sum()) for k in ks)
        assert ks and d_k > 0 and (n_k / d_k) ** 0.5 < 2e-2, (kind, (n_k / d_k) ** 0.5)
    P = unet.P
    trained = set(tr.names)
    fresh = Packed(unet_sd_np, "cpu", dtype=torch.float32)
    checked = 0
    for key, t in P.cache.items():
        kind, _, joined = key.partition(":")
        if kind not in ("mat", "vec", "fused", "fvec", "geglu", "gegluv") or not isinstance(t, torch.Tensor):
            continue
        ref = fresh._get(key)
        for r0, r1, n in P.row_ranges(key):
            if n not in trained:
                assert torch.equal(t[r0:r1], ref[r0:r1]), n
                checked += 1
    assert checked > 100
    for n in tr.unreached + ["conv_in.weight", "conv_out.weight", "down_blocks.0.resnets.0.temp_conv1.weight", "down_blocks.0.resnets.0.time_emb_proj.weight",
                             "down_blocks.0.attentions.0.transformer_blocks.0.norm1.weight", "time_embedding.linear_1.weight",
                             "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_k.weight"]:
        assert n not in trained and torch.equal(P.raw(n), sd[n]), n


# ------------------------------------------------------------------ layouts
def test_exported_shapes_checkpoint_round_trip_and_refused_names(emu, unet_sd_np, tmp_path):
    from safetensors.torch import save_file
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = tf.golden()
    mods = ("resnets.0.conv1", "resnets.0.conv_shortcut", "upsamplers.0.conv", "downsamplers.0.conv", "attentions.0.proj_in", "resnets.0.norm1", "conv_norm_out")
    unet = _unet(unet_sd_np)
    tr = util.UNetTuner(unet, trainable_modules=mods, lr=tf.LR)
    assert any(n.endswith("conv_shortcut.weight") for n in tr.names) and "conv_norm_out.weight" in tr.names
    for n in tr.names:
        packed = tr.masters[n]
        shape = tuple(unet_sd_np[n].shape)
        assert tuple(packed.shape) == ((shape[0], shape[2] * shape[3], shape[1]) if len(shape) == 4 else shape), n    # masters in the packed tap-major layout
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got = tr.export_state_dict()
    for n, v in got.items():
        assert tuple(v.shape) == tuple(unet_sd_np[n].shape) == tuple(unet.P.raw(n).shape) and v.is_contiguous(), n
        assert torch.equal(unet.P.raw(n), v), n                    # the live master, in the reference layout
        assert not torch.equal(v, torch.from_numpy(unet_sd_np[n])), n
    ck = tmp_path / "checkpoint-1"
    tr.save_checkpoint(ck)
    (tmp_path / "sd" / "unet").mkdir(parents=True)
    save_file({k: torch.from_numpy(v) for k, v in unet_sd_np.items() if not k.startswith("controlnet_adapter.")},
              str(tmp_path / "sd" / "unet" / "diffusion_pytorch_model.safetensors"))
    m = UNet2DConditionModel.from_pretrained(str(tmp_path / "sd"), subfolder="unet", resume_from_checkpoint=str(ck), device="cpu")
    for k, v in got.items():
        assert torch.equal(m.P.raw(k), v), k
    assert torch.equal(m.P.raw("conv_in.weight"), torch.from_numpy(unet_sd_np["conv_in.weight"]))


@pytest.mark.parametrize("kw,name", [
    (dict(trainable_modules=("resnets.0.temp_conv2",)), "temp_conv2"),
    (dict(trainable_modules=("conv1",)), "temp_conv1"),                                       # a bare suffix reaches the temporal convolution too: refused, by name
    (dict(trainable_modules=("attn1.to_q",), trainable_params=("mid_block.resnets.0.time_emb_proj.bias",)), "time_emb_proj"),
    (dict(trainable_modules=("time_embedding.linear_1",)), "time_embedding.linear_1"),
    (dict(trainable_modules=("conv_in",)), "conv_in.weight"),
    (dict(trainable_modules=("conv_out",)), "conv_out.bias"),
    (dict(trainable_modules=("transformer_blocks.0.norm2",)), "transformer_blocks.0.norm2"),  # LayerNorm affine parameters: fold sources
    (dict(trainable_modules=("norm_temp",)), "norm_temp"),
])
def test_still_refused_parameters_are_named(emu, unet_sd_np, kw, name):
    from motioneditor_amd import util
    with pytest.raises(NotImplementedError, match=re.escape(name)) as e:
        util.UNetTuner(_unet(unet_sd_np), **kw)
    assert "later change" in str(e.value)


# ------------------------------------------------------------------ the ABI table of include/motioned_tune.h
LAUNCHING = {"me_conv_dw", "me_groupnorm_bwd_params", "me_refresh_ups4"}


def test_tune_symbols_are_declared_exported_and_apart_from_the_other_tables():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    assert "tune.hip" in build.SOURCES
    assert not set(capi.TUNE_SYMBOLS) & (set(capi.SYMBOLS) | set(capi.IO_SYMBOLS))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "motioned_tune.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.TUNE_SYMBOLS) == LAUNCHING | {"me_conv_dw_work_bytes", "me_conv_dw_splits", "me_groupnorm_bwd_params_work_bytes"}
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    bound = capi.lib()
    for name, (res, args) in capi.TUNE_SYMBOLS.items():
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype is res
    assert bound.me_abi_version() == capi.ABI_VERSION == 9
    step_header = (ROOT / "include" / "motioned.h").read_text()
    assert not any(name in step_header for name in declared)
    fields = re.search(r"typedef struct me_conv_dw_args \{(.*?)\} me_conv_dw_args;", header, flags=re.S).group(1)
    c_names = [n for decl in fields.split(";") for n in re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl.strip())]
    assert c_names == [f[0] for f in capi.ConvDwArgs._fields_], c_names


def test_every_launching_tune_symbol_is_named_by_a_guard_case():
    """The rule of test_clip_io_cpu.py::test_every_io_symbol_is_named_by_a_guard_case for capi.TUNE_SYMBOLS: no exemptions among the entries that launch (the
    three size queries launch nothing and touch no memory)."""
    from motioneditor_amd import capi
    import test_guard_tune_gpu
    guarded = set()
    for syms in test_guard_tune_gpu.GUARDED.values():
        guarded |= set(syms)
    assert guarded <= set(capi.TUNE_SYMBOLS), sorted(guarded - set(capi.TUNE_SYMBOLS))
    assert not LAUNCHING - guarded, f"tuning entries without a guard case: {sorted(LAUNCHING - guarded)}"
    assert set(capi.TUNE_SYMBOLS) - guarded <= {"me_conv_dw_work_bytes", "me_conv_dw_splits", "me_groupnorm_bwd_params_work_bytes"}


def test_work_bytes_stay_inside_256_mib_for_every_convolution_of_the_unet():
    """8 frames x 64^2 latents: M = 8 * (64 >> level)^2; every (Cout, Cin) a 3x3 convolution of the UNet has (the up path's Cin carry the skip concatenation)."""
    from motioneditor_amd import capi
    L = capi.lib()
    shapes = {(32768, 320, 320), (8192, 320, 320), (8192, 640, 320), (8192, 640, 640), (2048, 640, 640), (2048, 1280, 640), (2048, 1280, 1280), (512, 1280, 1280),
              (512, 1280, 2560), (2048, 1280, 2560), (2048, 1280, 1920), (8192, 1280, 1280), (8192, 640, 1920), (8192, 640, 1280), (8192, 640, 960), (32768, 640, 640),
              (32768, 320, 960), (32768, 320, 640), (32768, 8, 320)}
    for M, N, K in shapes:
        b, s = L.me_conv_dw_work_bytes(M, N, K), L.me_conv_dw_splits(M, N, K)
        assert 0 < b <= 256 << 20 and b == s * N * 9 * K * 4 and s >= 1, (M, N, K, b, s)
    assert L.me_conv_dw_work_bytes(0, 8, 8) == 0 and L.me_conv_dw_splits(64, 0, 8) == 0


# ------------------------------------------------------------------ argument contract, without a device
def test_tune_argument_validation_returns_einval_without_a_device():
    from motioneditor_amd import capi
    L = capi.lib()
    P = 4096            # never dereferenced: every call below is refused before a launch

    def conv(**over):
        a = capi.ConvDwArgs()
        a.dY, a.X, a.dW, a.work = P, P, P, P
        a.M, a.N, a.K, a.lddy, a.ldx, a.dy_is_f16 = 2 * 5 * 7, 40, 72, 40, 72, 0
        a.Hin, a.Win, a.Hout, a.Wout, a.stride, a.ups, a.pad0, a.alpha = 5, 7, 5, 7, 1, 0, 0, 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return L.me_conv_dw(ctypes.byref(a), None)

    def gnp(dgamma=P, dbeta=P, x=P, ldx=64, gamma=P, beta=P, dy=P, lddy=64, rows=12, rpg=6, C=64, groups=32, work=P):
        return L.me_groupnorm_bwd_params(dgamma, dbeta, x, ldx, gamma, beta, dy, lddy, rows, rpg, C, groups, 1e-5, 1, 1.0, work, None)

    def ups(dst=P, master=P, N=8, K=16):
        return L.me_refresh_ups4(dst, master, N, K, None)

    conv_cases = [
        (lambda: conv(dY=None), b"null"), (lambda: conv(work=None), b"null"), (lambda: conv(X=P + 8), b"misaligned"), (lambda: conv(dW=P + 4), b"misaligned"),
        (lambda: conv(dY=P + 8), b"misaligned"), (lambda: conv(work=P + 4), b"misaligned"),
        (lambda: conv(N=44, lddy=44), b"multiples"), (lambda: conv(K=76, ldx=80), b"multiples"), (lambda: conv(ldx=76), b"multiples"), (lambda: conv(lddy=42), b"multiples"),
        (lambda: conv(lddy=44, dy_is_f16=1), b"multiples"), (lambda: conv(ldx=64), b"cover"),
        (lambda: conv(pad0=1), b"pad0"), (lambda: conv(ups=3, Hout=10, Wout=14, M=2 * 10 * 14), b"ups"), (lambda: conv(ups=2, Hout=10, Wout=14, M=2 * 10 * 14), b"ups"),
        (lambda: conv(stride=2, ups=1, Hout=5, Wout=7), b"stride 2 together with ups"), (lambda: conv(stride=3), b"stride"),
        (lambda: conv(M=2 * 5 * 7 + 8), b"whole images"), (lambda: conv(Hout=6), b"geometry"), (lambda: conv(stride=2), b"geometry"),
        (lambda: conv(ups=1), b"geometry"), (lambda: conv(Hin=0), b"geometry"), (lambda: conv(M=0), b"multiples")]
    gn_cases = [
        (lambda: gnp(dgamma=None, dbeta=None), b"null"), (lambda: gnp(x=None), b"null"), (lambda: gnp(work=None), b"null"), (lambda: gnp(rows=13), b"multiple of rows_per_group"),
        (lambda: gnp(C=60), b"channels"), (lambda: gnp(C=2568, groups=8, ldx=2568, lddy=2568), b"channels"), (lambda: gnp(groups=65), b"channels"),
        (lambda: gnp(ldx=68), b"strides"), (lambda: gnp(lddy=66), b"strides"), (lambda: gnp(ldx=56), b"strides"),
        (lambda: gnp(x=P + 8), b"misaligned"), (lambda: gnp(dy=P + 4), b"misaligned"), (lambda: gnp(gamma=P + 2), b"misaligned"), (lambda: gnp(dgamma=P + 2), b"misaligned")]
    ups_cases = [
        (lambda: ups(dst=None), b"bad arguments"), (lambda: ups(master=None), b"bad arguments"), (lambda: ups(K=18), b"multiple of 4"), (lambda: ups(N=0), b"bad arguments"),
        (lambda: ups(master=P + 4), b"misaligned"), (lambda: ups(dst=P + 2), b"misaligned")]
    for entry, cases in ((b"me_conv_dw:", conv_cases), (b"me_groupnorm_bwd_params:", gn_cases), (b"me_refresh_ups4:", ups_cases)):
        for i, (call, word) in enumerate(cases):
            rc, msg = call(), L.me_last_error()
            assert rc == capi.ME_EINVAL and word in msg and msg.startswith(entry), (entry, i, rc, msg)     # refused on the host, the message names the entry
    with pytest.raises(ValueError, match="me_conv_dw"):
        capi.check(conv(pad0=1), "me_conv_dw")
    # me_gemm_dw keeps refusing the 3x3 gather (tests/bwd_abi.py): the new entry is the only way in
    a = capi.GemmDwArgs()
    a.dY, a.X, a.dW, a.work, a.M, a.N, a.K, a.lddy, a.ldx, a.taps, a.tap, a.gather, a.alpha = P, P, P, P, 64, 64, 64, 64, 64, 9, 0, capi.GATHER_CONV3, 1.0
    assert L.me_gemm_dw(ctypes.byref(a), None) == capi.ME_EINVAL and b"dense and TemporalConv" in L.me_last_error()


def test_ops_gemm_dw_dispatches_the_conv_tuple_to_me_conv_dw(monkeypatch):
    """ops.gemm_dw(conv=...) no longer raises NotImplementedError: it fills me_conv_dw_args from the tape's conv tuple and makes ONE call for all nine taps."""
    from motioneditor_amd import capi, ops
    seen = []

    class FakeLib:
        def me_conv_dw_work_bytes(self, M, N, K):
            return 64

        def me_conv_dw(self, ref, stream):
            a = ref._obj
            seen.append((a.M, a.N, a.K, a.lddy, a.ldx, a.dy_is_f16, a.Hin, a.Win, a.Hout, a.Wout, a.stride, a.ups, a.pad0, a.alpha))
            return capi.ME_OK

    monkeypatch.setattr(capi, "lib", lambda: FakeLib())
    monkeypatch.setattr(ops, "_work", lambda n, dev, tag: torch.zeros(16))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_chk2d", lambda t, name: None)
    dy, x, dst = torch.zeros(2 * 4 * 5, 48)[:, :40], torch.zeros(2 * 7 * 9, 80, dtype=torch.float16)[:, :72], torch.zeros(40, 9, 72)
    assert ops.gemm_dw(dy, x, dst=dst, taps=9, K=72, M=40, alpha=0.5, conv=(7, 9, 4, 5, 2, 0)) is dst
    assert seen == [(40, 40, 72, 48, 80, 0, 7, 9, 4, 5, 2, 0, 0, 0.5)]
    with pytest.raises(ValueError, match="9"):
        ops.gemm_dw(dy, x, dst=torch.zeros(40, 1, 72), taps=1, K=72, M=40, conv=(7, 9, 4, 5, 2, 0))
