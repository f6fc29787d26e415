"""The nearest-2x upsampler convolutions as four 2x2-tap convolutions (me_gemm gather mode ups = 3), the parts that need no GPU: the fold table,
the packed layout and rounding of weights.Packed.mat_ups, and its life cycle -- rebuilt after Packed.update, never handed out while a trainer
rewrites the plain packing in place -- through graph.conv3x3's routing."""
import types

import pytest
import torch

from ups_fold_ref import conv_fold_ref, conv_ups_ref, rel_l2

from motioneditor_amd.models import graph
from motioneditor_amd.weights import Packed


def _w(n, k, seed):
    return torch.randn(n, k, 3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7)])
def test_fold_table_is_exact_in_fp64(H, W):
    """Four 2x2-tap convolutions with the UNROUNDED folded weights equal conv2d(interpolate(x, 2, 'nearest'), W, padding = 1): N != K, two images."""
    n_img, K, N = 2, 5, 3
    x = torch.randn(n_img * H * W, K, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    w = _w(N, K, 2)
    want = conv_ups_ref(x, Packed._as_taps(w), n_img, H, W)
    got = conv_fold_ref(x, Packed.fold_ups(w), n_img, H, W)
    assert got.shape == want.shape == (n_img * 4 * H * W, N)
    err = float((got - want).abs().max())
    print(f"fold {H}x{W}: max abs error {err:.3e}")
    assert err <= 1e-12


def test_fold_weights_are_sums_of_1_2_or_4_taps():
    w = torch.ones(1, 1, 3, 3, dtype=torch.float64)
    f = Packed.fold_ups(w).reshape(2, 2, 2, 2)     # [py, px, ty, tx]
    for py in range(2):
        for px in range(2):
            rows = [1, 2] if py == 0 else [2, 1]
            cols = [1, 2] if px == 0 else [2, 1]
            assert f[py, px].tolist() == [[rows[0] * cols[0], rows[0] * cols[1]], [rows[1] * cols[0], rows[1] * cols[1]]]
    assert float(f.sum()) == 36.0                  # every one of the 9 taps lands once in each of the 4 parities


def test_mat_ups_layout_and_rounding():
    N, K = 6, 8
    w = _w(N, K, 3).float()
    P = Packed({"c.weight": w}, "cpu")
    m = P.mat_ups("c.weight")
    assert m.shape == (N, 16, K) and m.dtype == torch.float16 and m.is_contiguous()
    # index 4 p + t, the fold table written out: rows fold by py, columns by px
    rowsets = {0: ([0], [1, 2]), 1: ([0, 1], [2])}      # py -> (ky of ty = 0, ky of ty = 1)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    s = torch.zeros(N, K)
                    for ky in rowsets[py][ty]:
                        for kx in rowsets[px][tx]:
                            s = s + w[:, :, ky, kx]                # fp32 sums ...
                    got = m[:, 4 * (2 * py + px) + 2 * ty + tx]
                    assert torch.equal(got, s.to(torch.float16)), (py, px, ty, tx)   # ... rounded to fp16 once
    assert P.mat_ups("c.weight") is m                     # packed once, under its own key
    assert "ups4:c.weight" in P.cache


def _fake_ops(calls):
    """A stand-in backend that offers the folded mode: gemm computes either form in fp64 from its definition and notes which one it was asked for."""
    def gemm(x, w, *, M=None, bias=None, conv=None, **kw):
        H, W, ho, wo, stride, ups = conv[:6]
        n_img = M // (ho * wo)
        calls.append((ups, tuple(w.shape)))
        if ups == 0:
            return torch.zeros(M, w.shape[0])
        y =conv_fold_ref(x, w, n_img, H, W) if ups == 3 else conv_ups_ref(x, w, n_img, H, W)
        return (y + bias.double()[None]).float()
    return types.SimpleNamespace(UPS_FOLD=True, gemm=gemm)


def _ref(x, w, b, n_img, H, W):
    return conv_ups_ref(x, Packed._as_taps(w), n_img, H, W) + b.double()[None]


def test_update_then_forward_uses_the_rebuilt_fold(monkeypatch):
    """update -> forward: the folded tensor of a replaced parameter is re-packed (the stale-cache defect of a derived weight must not come back)."""
    n_img, H, W, K, N = 2, 3, 4, 8, 8
    calls = []
    monkeypatch.setattr(graph, "ops", _fake_ops(calls))
    monkeypatch.delenv("ME_UPS_FOLD", raising=False)
    w0, w1, b = _w(N, K, 4).float(), _w(N, K, 5).float(), torch.randn(N, generator=torch.Generator().manual_seed(6))
    P = Packed({"up.weight": w0, "up.bias": b}, "cpu")
    x = torch.randn(n_img * H * W, K, generator=torch.Generator().manual_seed(7)).half()
    act = graph.Act(x, n_img, 1, H, W)
    tol = 2e-3      # fp16 rounding of weights (and bias) of 8 x 9 products: ~ 2^-11 per weight
    y0 = graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1] == (3, (N, 16, K)) and (y0.h, y0.w) == (2 * H, 2 * W)
    assert rel_l2(y0.t, _ref(x, w0, b, n_img, H, W)) <= tol
    P.update("up.weight", w1)
    assert "ups4:up.weight" not in P.cache
    y1 = graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1] == (3, (N, 16, K))
    e_new, e_old = rel_l2(y1.t, _ref(x, w1, b, n_img, H, W)), rel_l2(y1.t, _ref(x, w0, b, n_img, H, W))
    print(f"after update: {e_new:.3e} from the new weight, {e_old:.3e} from the old one")
    assert e_new <= tol and e_old > 0.5


def test_fold_is_not_used_where_a_trainer_rewrites_the_weight_in_place(monkeypatch):
    """rehome (AdapterTrainer) and live masters (the background tuner) refresh the PLAIN packing in place: conv3x3 then keeps the 9-tap form, so no
    folded copy can go stale; so it does with ME_UPS_FOLD=0, while a tape records, and on a backend without the mode."""
    n_img, H, W, K, N = 1, 2, 2, 8, 8
    calls = []
    fake = _fake_ops(calls)
    monkeypatch.setattr(graph, "ops", fake)
    monkeypatch.delenv("ME_UPS_FOLD", raising=False)
    w0, b = _w(N, K, 8).float(), torch.zeros(N)
    x = torch.randn(n_img * H * W, K, generator=torch.Generator().manual_seed(9)).half()
    act = graph.Act(x, n_img, 1, H, W)

    P = Packed({"up.weight": w0, "up.bias": b}, "cpu")
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1][0] == 3
    store = torch.zeros(N * 9 * K, dtype=torch.float16)
    P.rehome("mat:up.weight", store)
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1] == (1, (N, 9, K)) and "ups4:up.weight" not in P.cache

    P = Packed({"up.weight": w0, "up.bias": b}, "cpu")
    P.live["up.weight"] = lambda: w0
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1] == (1, (N, 9, K))

    P = Packed({"up.weight": w0, "up.bias": b}, "cpu")
    monkeypatch.setenv("ME_UPS_FOLD", "0")
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1][0] == 1
    monkeypatch.setenv("ME_UPS_FOLD", "1")              # read per call
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1][0] == 3
    fake.recording = True
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1][0] == 1
    fake.recording = False
    fake.UPS_FOLD = False
    graph.conv3x3(P, "up", act, ups=1)
    assert calls[-1][0] == 1
    graph.conv3x3(P, "up", act, ups=0)                  # a plain 3x3 convolution never folds
    fake.UPS_FOLD = True
    graph.conv3x3(P, "up", graph.Act(x, n_img, 1, H, W), ups=0)
    assert calls[-1] == (0, (N, 9, K))
