"""Guard-band cases for the tuning entries of include/motioned_tune.h (capi.TUNE_SYMBOLS) on a real MI355X, through the protocol of tests/guard.py: three
launches on the same addresses with the input surroundings NaN / 0 / 6e4, accumulated-into operands restored between them, every allocation's surroundings
bitwise intact, the wrappers' scratch NaN-filled before every launch.  me_conv_dw's gather reads zero rows for taps outside an image: with NaN above and below
the activation view, a tap that took the neighbouring pixel row, image or allocation instead would show.

GUARDED maps every case to the symbols it drives; tests/test_tune_conv_cpu.py checks it against capi.TUNE_SYMBOLS without a GPU, and on the GPU the decorator
counts the calls, so a case that stops reaching a symbol it names fails."""
import fnmatch
import functools

import pytest
import torch

import emu_tune_ops as emu
import guard
import tune_fixture as tf
from guard import check, embed_in, run_guarded

pytestmark = pytest.mark.gpu

GUARDED = {}


def guards(*symbols):
    def deco(fn):
        GUARDED[fn.__name__] = symbols

        @functools.wraps(fn)
        def run(*a, **kw):
            from motioneditor_amd import capi
            L, calls, saved = capi.lib(), dict.fromkeys(symbols, 0), {}
            for s in symbols:
                saved[s] = getattr(L, s)

                def spy(*args, _s=s):
                    calls[_s] += 1
                    return saved[_s](*args)
                setattr(L, s, spy)
            try:
                fn(*a, **kw)
            finally:
                for s in symbols:
                    setattr(L, s, saved[s])
            assert all(calls.values()), f"the case never reached {[s for s, n in calls.items() if not n]}"
        return run
    return deco


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


def E(t, **kw):
    return embed_in(t, device="cuda", **kw)


def V(t, **kw):
    return embed_in(t, device="cuda", contiguous=True, **kw)


def kernel_is(ops, want):
    got = ops._last_kernel()
    print("kernel:", got)
    assert fnmatch.fnmatchcase(got, want), f"the case was written for {want}, the launch took {got}"


@pytest.mark.parametrize("mode,n_img,Hin,Win,N,K,stride,ups", [("stride1", 2, 5, 7, 40, 72, 1, 0), ("stride2", 2, 7, 9, 40, 72, 2, 0), ("ups", 2, 3, 5, 72, 40, 1, 1),
                                                              ("stride1_f16", 3, 4, 4, 136, 64, 1, 0)])
@guards("me_conv_dw")
def test_guard_conv_dw(ops, mode, n_img, Hin, Win, N, K, stride, ups):
    x, dy, base, conv, M = tf.conv_dw_inputs(n_img, Hin, Win, N, K, stride, ups, seed=3)
    dyc = dy.half() if mode.endswith("f16") else dy
    ins = {"dy": E(dyc), "x": E(x), "dst": V(base)}
    got = run_guarded(lambda: ops.gemm_dw(ins["dy"], ins["x"], dst=ins["dst"], taps=9, K=K, M=M, conv=conv), ins, {}, inout=["dst"],
                      before=lambda: guard.poison_scratch(ops))
    kernel_is(ops, "conv_dw_kernel<f16>" if mode.endswith("f16") else "conv_dw_kernel<f32>")
    want = emu.gemm_dw(dy.half().float(), x, dst=base.clone(), taps=9, K=K, M=M, conv=conv)
    check(got["dst"].cpu() - base, want - base, f"guard conv_dw {mode}")


@pytest.mark.parametrize("Cc,rpg,nsg,silu", [(320, 96, 2, True), (640, 50, 3, False), (2560, 70, 1, True)])
@guards("me_groupnorm_bwd_params")
def test_guard_groupnorm_bwd_params(ops, Cc, rpg, nsg, silu):
    x, gm, bt, dy, g0, b0 = tf.gn_inputs(Cc, rpg, nsg, seed=4)
    ins = {"x": E(x), "gamma": V(gm), "beta": V(bt), "dy": E(dy), "dgamma": V(g0), "dbeta": V(b0)}
    got = run_guarded(lambda: ops.groupnorm_bwd(ins["x"], ins["gamma"], ins["beta"], ins["dy"], rows_per_group=rpg, eps=1e-5, silu=silu, dgamma=ins["dgamma"],
                                                dbeta=ins["dbeta"]), ins, {}, inout=["dgamma", "dbeta"], before=lambda: guard.poison_scratch(ops))
    kernel_is(ops, "gn_params_part_kernel")
    wg, wb = g0.clone(), b0.clone()
    emu.groupnorm_bwd(x, gm, bt, dy, rows_per_group=rpg, eps=1e-5, silu=silu, dgamma=wg, dbeta=wb)
    check(got["dgamma"].cpu() - g0, wg - g0, f"guard groupnorm_bwd_params dgamma C={Cc}")
    check(got["dbeta"].cpu() - b0, wb - b0, f"guard groupnorm_bwd_params dbeta C={Cc}")


@guards("me_refresh_ups4")
def test_guard_refresh_ups4(ops):
    from motioneditor_amd.weights import Packed
    N, K = 40, 72
    w = torch.randn(N, K, 3, 3, generator=torch.Generator().manual_seed(5)) * 0.1
    ins = {"master": V(Packed._as_taps(w).contiguous()), "dst": V(guard.rnd(N, 16, K, seed=6))}
    table = ops.refresh_table([(ins["master"], ins["dst"], None, None, None, None, None)])
    got = run_guarded(lambda: ops.refresh_weights(table), ins, {}, inout=["dst"])
    kernel_is(ops, "refresh_ups4_kernel")
    assert torch.equal(got["dst"].cpu(), Packed.fold_ups(w).half())
