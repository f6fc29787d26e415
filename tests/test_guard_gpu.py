"""Guard-band cases on a real MI355X: every kernel-launching entry point of the C ABI on views inside allocations the test owns (tests/guard.py).

Each case runs the protocol of guard.run_guarded -- three launches on the same addresses with the input surroundings NaN / 0 / 6e4 -- and asserts (1) finite,
bitwise equal results, (2) intact sentinels around every output, (3) unchanged inputs, (4) the bound of tests/test_kernels_gpu.py's check() against the fp32
emulation (REL_L2 = 2e-3, MAX_REL = 2e-2, restated in guard.py), (5) the kernel form through ops._last_kernel() where the entry point records it.  Views are
16-byte but not 32-byte aligned, 2-D views have a leading dimension larger than their width, K / V views end exactly at the last key.  Cases that take
scratch run with the scratch refilled with NaN before every launch.

Out of reach: a stray read whose value is discarded; strays of more than one tile (256 rows / 64 columns / one weight panel) beyond a view; a stray read of
seg_mode (its surroundings are 0 in all three launches: another mode could name a path whose operands are NULL); buffers a wrapper allocates per call and
the test cannot fill (attention_bwd's `delta`, the fp16 copies and transposed weights inside gemm_dx).  _last_kernel() names the kernel template and its tile,
not the epilogue specialisation (EPI 0 / 2 / 4 / 6 / 12 / generic) nor STAGE_BUF against STAGE_GLDS: those are selected by the terms and the K of a case
(K % 64 == 0: buffer staging) and are not witnessed.
No case passes a pointer or a size the ABI does not allow: whatever a wrong kernel could touch lies inside the test's own allocations.

GUARDED maps every case to the ABI symbols it drives (tests/test_guard_cpu.py checks it against capi.SYMBOLS without a GPU); on the GPU the decorator also
counts the calls, so a case that stops reaching a symbol it names fails."""
import ctypes as C
import fnmatch
import functools

import pytest
import torch

import emu_clip_ops as emu_clip
import emu_ops as emu
import guard
from guard import check, embed_in, rnd, run_guarded, scratch_independent, sentinel_out

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
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
    """A 2-D row view (or head-major panels) in guards."""
    return None if t is None else embed_in(t, device="cuda", **kw)


def V(t, **kw):
    """What the ABI wants contiguous (weights, vectors, tables, flat buckets) between guard elements."""
    return None if t is None else embed_in(t, device="cuda", contiguous=True, **kw)


def O(shape, dtype=F16, **kw):
    return sentinel_out(shape, dtype, device="cuda", **kw)[0]


def lib():
    from motioneditor_amd import capi
    return capi.lib()


def call(ops, name, *args):
    from motioneditor_amd import capi
    capi.check(getattr(capi.lib(), name)(*args, ops._stream()), name)


def kernel_is(ops, want):
    got = ops._last_kernel()
    print("kernel:", got)
    assert fnmatch.fnmatchcase(got, want), f"the case was written for {want}, the launch took {got}"


def _acc0(shape, seed=99, scale=0.5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _poison(ops):
    return lambda: guard.poison_scratch(ops)


# ------------------------------------------------------------------ me_gemm
def gemm_case(ops, x, w, kernel, *, name, inplace=False, **kw):
    """x, w and every tensor of kw on the CPU: embedded here, run through ops.gemm(out=sentinel view), compared with emu.gemm on the same tensors.  Weights get
    a guard of one 320-row panel, so a column tile that loads rows past N reads poison."""
    N, taps, K = w.shape
    M = kw.get("M") or x.shape[0]
    n_out = N // 2 if kw.get("geglu") else N
    ins = {"x": E(x), "w": V(w, row_guard=320 * taps, col_guard=K), "bias": V(kw.get("bias")), "rowvec": E(kw.get("rowvec")), "res": E(kw.get("res")), "res2": E(kw.get("res2"))}
    outs = {} if inplace else {"out": O((M, n_out))}
    out = ins["res"] if inplace else outs["out"]
    gkw = {k: (ins[k] if k in ins else v) for k, v in kw.items()}
    got = run_guarded(lambda: ops.gemm(ins["x"], ins["w"], out=out, **gkw), ins, outs, inout=["res"] if inplace else [], before=_poison(ops))
    kernel_is(ops, kernel)
    check(got["res" if inplace else "out"], emu.gemm(x, w, **kw), name)


GEMM_DENSE = {   # name: (M, N, K, terms, kernel) -- the tile families of me_gemm's dispatch at the smallest grids that select them, M off the tile
    "128x64 tile, K tail": (8, 64, 8, "none", "gemm_kernel<128,64>"),
    "128x128 tile": (128 * 30 + 7, 1024, 64, "bias+res", "gemm_kernel<128,128>"),
    "128x160 tile": (300, 480, 64, "bias+rowvec+res+res2", "gemm_kernel<128,160>"),
    "256x320 tile": (256 * 519 + 77, 320, 64, "bias+res", "gemm_kernel<256,320>"),
    "N = 4": (37, 4, 320, "bias", "gemm_kernel<128,128>"),
    "in place": (260, 320, 320, "inplace", "gemm_kernel<128,64>"),
    "shared residual rows": (3 * 200 + 7, 320, 64, "res_rows", "gemm_kernel<128,64>"),
    "split-K": (3000, 1280, 2560, "bias+rowvec+res+res2+silu", "gemm_kernel<128,128>+splitk"),
    "8-phase 256-row, M and K tails": (256 * 260 + 77, 640, 192, "bias+res", "gemm8p_kernel<256,320,false>"),
    "8-phase 192-row, M tail": (24000 - 40, 1280, 512, "bias+res", "gemm8p_kernel<192,320,false>"),
    "8-phase 128-row, M tail": (6144 - 40, 1280, 1280, "bias+res", "gemm8p_kernel<128,320,false>"),
}


def _dense_case(ops, case, table):
    M, N, K, terms, kernel = table[case]
    x, w = rnd(M, K, seed=1), rnd(N, 1, K, seed=2, scale=K ** -0.5)
    kw = {}
    if "bias" in terms or terms == "inplace":
        kw["bias"] = rnd(N, seed=3)
    if "rowvec" in terms:
        kw.update(rowvec=rnd(8, N, seed=4), rows_per_vec=(M + 7) // 8)
    if "res" in terms.split("+") or terms == "inplace":
        kw["res"] = rnd(M, N, seed=5)
    if "res2" in terms:
        kw["res2"] = rnd(M, N, seed=6)
    if "silu" in terms:
        kw["act"] = 2
    if terms == "res_rows":
        kw.update(res=rnd(200, N, seed=5), res_rows=200)
    gemm_case(ops, x, w, kernel, name=f"guard gemm {case}", inplace=terms == "inplace", **kw)


@pytest.mark.parametrize("case", list(GEMM_DENSE))
@guards("me_gemm")
def test_guard_gemm_dense(ops, case):
    _dense_case(ops, case, GEMM_DENSE)


# ME_GEMM_STAGE=reg (global -> VGPR -> padded LDS, the first implementation, kept for A/B runs) is read once per process: these run in a fresh child.
GEMM_REG = {
    "reg 128x128, M, N and K tails": (300, 200, 64 + 8, "bias+res", "gemm_kernel<128,128,reg>"),
    "reg 128x64, M and K tails": (140, 192, 64 + 8, "bias+rowvec+res+res2", "gemm_kernel<128,64,reg>"),
    "reg in place": (260, 320, 320, "inplace", "gemm_kernel<128,64,reg>"),
}


def reg_stage_child():
    """Runs in the child process of test_guard_gemm_register_staged_kernels_in_a_fresh_process."""
    import os
    assert os.environ.get("ME_GEMM_STAGE") == "reg"
    from motioneditor_amd import capi, ops
    capi.lib()
    for case in GEMM_REG:
        _dense_case(ops, case, GEMM_REG)
    Cin, Cout, H, W, nimg = 320, 640, 8, 8, 3      # a gather form: the stride-2 convolution
    x, w = rnd(nimg * H * W, Cin, seed=1), rnd(Cout, 9, Cin, seed=2, scale=(9 * Cin) ** -0.5)
    gemm_case(ops, x, w, "gemm_kernel<128,128,reg>", name="guard gemm reg conv stride 2", M=nimg * 16, conv=(H, W, 4, 4, 2, 0), bias=rnd(Cout, seed=3))
    print("reg stage: all cases passed")


def test_guard_gemm_register_staged_kernels_in_a_fresh_process(ops):
    import os
    import subprocess
    import sys
    from pathlib import Path
    tests = Path(__file__).resolve().parent
    code = f"import sys; sys.path[:0] = [{str(tests.parent)!r}, {str(tests)!r}]; import test_guard_gpu as T; T.reg_stage_child()"
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "ME_GEMM_STAGE": "reg"}, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "reg stage: all cases passed" in r.stdout, f"child exit {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


GUARDED["test_guard_gemm_register_staged_kernels_in_a_fresh_process"] = ("me_gemm",)      # (the calls happen in the child: not counted here)


# (240 tiles of 256 x 256 are the smallest grid that takes the 8-phase GEGLU kernel: 24 row tiles at N / 2 = 1280, the last one ragged)
@pytest.mark.parametrize("M,kernel", [(300, "gemm_kernel<128,64>"), (256 * 23 + 77, "gemm8p_kernel<256,256,false>")])
@guards("me_gemm")
def test_guard_gemm_geglu(ops, M, kernel):
    """Both GEGLU forms.  Measured on an MI355X: rel-L2 3.5e-5, max/mean 1.2e-2 at both shapes.  The max/mean figure of a * gelu(g) grows with the number of
    outputs (heavy-tailed products, one fp16 ulp of the largest against the mean): 2.4e-2 at M = 33005, which is why the case stays at the smallest grid that
    selects the 8-phase kernel."""
    from motioneditor_amd.weights import Packed
    Cc = 320
    P = Packed({"w": torch.randn(8 * Cc, Cc, generator=torch.Generator().manual_seed(1)) * Cc ** -0.5, "b": torch.randn(8 * Cc, generator=torch.Generator().manual_seed(2)) * 0.1}, "cpu")
    gemm_case(ops, rnd(M, Cc, seed=3), P.geglu_mat("w"), kernel, name="guard gemm geglu", bias=P.geglu_vec("b"), geglu=True)


GEMM_GATHER = {   # name: (Cin, Cout, H, W, stride, ups, pad0, nimg, kernel)
    "conv stride 1": (320, 320, 8, 8, 1, 0, 0, 5, "gemm_kernel<128,64>"),
    "conv stride 2": (320, 640, 8, 8, 2, 0, 0, 3, "gemm_kernel<128,64>"),
    "conv upsampled": (640, 640, 4, 4, 1, 1, 0, 3, "gemm_kernel<128,64>"),
    "conv zero-stuffed": (64, 128, 8, 12, 1, 2, 0, 2, "gemm_kernel<128,64>"),
    "conv pad0": (32, 96, 16, 16, 2, 0, 1, 2, "gemm_kernel<128,128>"),
    "conv N = 4": (320, 4, 8, 8, 1, 0, 0, 4, "gemm_kernel<128,128>"),
    "conv small channels": (16, 16, 24, 20, 1, 0, 0, 3, "gemm_kernel<128,128>"),
    "conv halo tile": (64, 640, 32, 32, 1, 0, 0, 64, "conv3_halo_kernel"),
    "conv stride 2, 8-phase gather": (128, 320, 32, 32, 2, 0, 0, 512, "gemm8p_kernel<256,320,true>"),
    "conv upsampled, 8-phase gather": (64, 320, 8, 8, 1, 1, 0, 512, "gemm8p_kernel<256,320,true>"),
    "conv stride 2, 192-row 8-phase gather": (64, 320, 32, 32, 2, 0, 0, 145, "gemm8p_kernel<192,320,true>"),      # 194 tiles of 192 rows, the last one ragged
}


@pytest.mark.parametrize("case", list(GEMM_GATHER))
@guards("me_gemm")
def test_guard_gemm_conv3x3(ops, case):
    Cin, Cout, H, W, stride, ups, pad0, nimg, kernel = GEMM_GATHER[case]
    if ups == 2:
        ho, wo = 2 * H, 2 * W
    elif pad0:
        ho, wo = H // 2, W // 2
    else:
        ho, wo = ((H << ups) - 1) // stride + 1, ((W << ups) - 1) // stride + 1
    M = nimg * ho * wo
    x, w = rnd(nimg * H * W, Cin, seed=1), rnd(Cout, 9, Cin, seed=2, scale=(9 * Cin) ** -0.5)
    kw = dict(M=M, conv=(H, W, ho, wo, stride, ups) + ((1,) if pad0 else ()), bias=rnd(Cout, seed=3))
    if kernel == "conv3_halo_kernel":
        kw.update(res=rnd(M, Cout, seed=4), rowvec=rnd(nimg, Cout, seed=5), rows_per_vec=H * W, act=2)
    gemm_case(ops, x, w, kernel, name=f"guard gemm {case}", **kw)


@pytest.mark.parametrize("form", ["plain", "8-phase gather", "sharded with halo rows", "row range"])
@guards("me_gemm")
def test_guard_gemm_tconv(ops, form):
    Cc, npix, nb = 320, 4, 2
    w, bias = rnd(Cc, 3, Cc, seed=2, scale=(3 * Cc) ** -0.5), rnd(Cc, seed=3)
    if form == "plain":
        rows = nb * 16 * npix
        gemm_case(ops, rnd(rows, Cc, seed=1), w, "gemm_kernel<128,64>", name="guard tconv", bias=bias, tconv=(16, npix, 8), res=rnd(rows, Cc, seed=4))
        return
    if form == "8-phase gather":      # (grids of >= 512 tiles of 256 x 320; the per-batch-entry row vector and the residual of temp_conv1)
        frames, npix, nb = 16, 64, 128
        rows = nb * frames * npix
        gemm_case(ops, rnd(rows, Cc, seed=1), w, "gemm8p_kernel<256,320,true>", name="guard tconv 8-phase", bias=bias, tconv=(frames, npix, 8), rowvec=rnd(nb, Cc, seed=5),
                  rows_per_vec=frames * npix, res=rnd(rows, Cc, seed=4))
        return
    f_loc, f_tot, frame0 = 8, 24, 8
    rows, hb = nb * f_loc * npix, nb * npix
    x = rnd(rows + 2 * hb, Cc, seed=1)                              # [local | prev halo | next halo]: the halo rows are the LAST rows of the view
    tc = (f_loc, npix, 24, frame0, f_tot, rows, rows + hb)
    if form != "row range":
        gemm_case(ops, x, w, "gemm_kernel<128,64>", name="guard tconv sharded", M=rows, bias=bias, tconv=tc, res=rnd(rows, Cc, seed=4))
        return
    # only the rows [lo, hi) of the M-row problem are written: the output view is an in-out operand whose other rows must keep their bits
    lo, hi = npix, (f_loc - 1) * npix
    res, old = rnd(rows, Cc, seed=4), rnd(rows, Cc, seed=7)
    ins = {"x": E(x), "w": V(w, row_guard=320 * 3, col_guard=Cc), "bias": V(bias), "res": E(res), "out": E(old)}
    got = run_guarded(lambda: ops.gemm(ins["x"], ins["w"], M=rows, tconv=tc, bias=ins["bias"], res=ins["res"], out=ins["out"], row_range=(lo, hi)), ins, {}, inout=["out"])
    kernel_is(ops, "gemm_kernel<128,64>")
    want = emu.gemm(x, w, M=rows, bias=bias, tconv=tc, res=res)
    check(got["out"][lo:hi], want[lo:hi], "guard tconv row range")
    assert torch.equal(got["out"][:lo].cpu(), old[:lo]) and torch.equal(got["out"][hi:].cpu(), old[hi:]), "rows outside the range were written"


def _gemm_args(x, w, out, M, **fields):
    from motioneditor_amd import capi
    a = capi.GemmArgs()
    N, taps, K = w.shape
    a.X, a.W, a.C, a.M, a.N, a.K, a.ldx, a.ldc, a.alpha = x.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, x.stride(0), out.stride(0), 1.0
    for k, v in fields.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("M", [300, 256 * 520 - 3])
@guards("me_gemm", "me_ln_stats")
def test_guard_gemm_head_major_panels_ln_fold_and_row_sums(ops, M):
    """The q | k | v projection as the step issues it: LayerNorm folded in (ln statistics, colsum, cvec as guarded fp32 inputs), q as rows and k | v as head-major
    panels (the second output, guards between the heads); then a projection that leaves the row sums of its output behind (ln_out, a guarded fp32 output).
    Driven through the ABI: ops.gemm allocates the panels and the row sums itself."""
    Cc, dh = 320, 40
    N = 3 * Cc
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, Cc, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + 4.0 * torch.randn(M, 1, generator=g)).half()
    gamma, beta = (1.0 + 0.2 * torch.randn(Cc, generator=g)).half(), (0.1 * torch.randn(Cc, generator=g)).half()
    w = rnd(N, 1, Cc, seed=2, scale=Cc ** -0.5)
    wq = (w.float() * gamma.float()[None, None, :]).half()
    cs, cv = wq.float().sum(dim=(1, 2)), w.float()[:, 0, :] @ beta.float()
    xg = E(x)
    st = O((1, M, 2), F32, contiguous=True)
    stats = run_guarded(lambda: call(ops, "me_ln_stats", xg.data_ptr(), xg.stride(0), M, Cc, st.data_ptr(), st.stride(0)), {"x": xg}, {"st": st})["st"]
    kernel_is(ops, "ln_stats")
    ins = {"x": xg, "w": V(wq, row_guard=320, col_guard=Cc), "stats": V(stats), "colsum": V(cs), "cvec": V(cv)}
    outs = {"q": O((M, Cc)), "kv": O((16, M, dh))}
    a = _gemm_args(ins["x"], ins["w"], outs["q"], M, C2=outs["kv"].data_ptr(), c2_col0=Cc, c2_dh=dh, c2_hs=outs["kv"].stride(0), ln_stats=ins["stats"].data_ptr(),
                   ln_colsum=ins["colsum"].data_ptr(), ln_cvec=ins["cvec"].data_ptr(), ln_eps=1e-5, ln_parts=1, ln_stride=ins["stats"].stride(0))
    got = run_guarded(lambda: call(ops, "me_gemm", C.byref(a)), ins, outs)
    kernel_is(ops, "gemm8p_kernel<256,320,false>" if M > 100000 else "gemm_kernel<128,64>")
    want = emu.gemm(emu.layernorm(x.float(), gamma, beta), w.float())
    check(got["q"], want[:, :Cc], "guard ln-folded q")
    check(got["kv"].permute(1, 0, 2).reshape(M, 2 * Cc), want[:, Cc:], "guard ln-folded head-major k | v")
    # ln_out: the partial row sums of the rows this projection writes
    w2, res = rnd(Cc, 1, Cc, seed=5, scale=Cc ** -0.5), rnd(M, Cc, seed=6)
    ins = {"x": xg, "w": V(w2, row_guard=320, col_guard=Cc), "res": E(res)}
    outs = {"y": O((M, Cc)), "sums": O((1, M, 2), F32, contiguous=True)}
    a2 = _gemm_args(ins["x"], ins["w"], outs["y"], M, res=ins["res"].data_ptr(), ldr=ins["res"].stride(0), ln_out=outs["sums"].data_ptr(), ln_out_stride=outs["sums"].stride(0))
    got = run_guarded(lambda: call(ops, "me_gemm", C.byref(a2)), ins, outs)
    kernel_is(ops, "gemm8p_kernel<256,320,false>" if M > 100000 else "gemm_kernel<128,64>")
    check(got["y"], emu.gemm(x, w2, res=res), "guard gemm ln_out y")
    yf = got["y"].float()
    check(got["sums"][0, :, 0], yf.sum(-1), "guard gemm ln_out sums")
    check(got["sums"][0, :, 1], (yf * yf).sum(-1), "guard gemm ln_out sums of squares")


@guards("me_gemm")
def test_guard_gemm_split_k_after_a_larger_launch(ops):
    """Grow-only split-K scratch: a larger split launch first, then the smaller one, against the smaller one on NaN-filled scratch."""
    def mk(M, K, seed, kernel):
        x, w = E(rnd(M, K, seed=seed)), V(rnd(1280, 1, K, seed=seed + 1, scale=K ** -0.5))

        def run():
            y = ops.gemm(x, w)
            kernel_is(ops, kernel)
            return y
        return run
    scratch_independent(mk(1000, 2048, 1, "gemm_kernel<128,64>+splitk"), _poison(ops), run_larger=mk(3000, 2560, 3, "gemm_kernel<128,128>+splitk"))


# ------------------------------------------------------------------ me_conv_small
@pytest.mark.parametrize("Cin,Cout,n_img,H,W,frames,f16in", [(4, 320, 4, 7, 9, 2, False), (3, 16, 4, 16, 16, 0, False), (3, 128, 2, 24, 40, 0, True),
                                                             (4, 16, 3, 7, 9, 0, False), (4, 200, 2, 7, 9, 0, True), (3, 512, 2, 7, 9, 0, False)])
@guards("me_conv_small")
def test_guard_conv_small(ops, Cin, Cout, n_img, H, W, frames, f16in):
    """Both kernels at Cin 3 and 4 (the plain one for 16 outputs and, in slices of 80 channels, for widths the tile kernel does not take: 200 = 80 + 80 + 40, 512;
    the 64-pixel tile kernel for wide outputs with a pixel count off the tile), fp32 and fp16 input, the 5-D strides."""
    from motioneditor_amd import capi
    g = torch.Generator().manual_seed(18)
    wt, bias = torch.randn(Cout, 9, Cin, generator=g) * 0.2, torch.randn(Cout, generator=g) * 0.1
    if frames:
        x = torch.randn(n_img // frames, Cin, frames, H, W, generator=g)
        kw = dict(n_img=n_img, Cin=Cin, H=H, Wd=W, img_stride=Cin * frames * H * W, ch_stride=frames * H * W, frames=frames, frame_stride=H * W)
    else:
        x = torch.randn(n_img, Cin, H, W, generator=g)
        kw = dict(n_img=n_img, Cin=Cin, H=H, Wd=W, img_stride=Cin * H * W, ch_stride=H * W)
    if f16in:
        x = x.half()
    kw["silu"] = Cout == 16
    ins = {"x": V(x), "w": V(wt), "bias": V(bias)}
    out = O((n_img * H * W, Cout), contiguous=True)      # (the ABI has no leading dimension for this output)
    a = capi.ConvSmallArgs()
    a.inp, a.W, a.bias, a.out = ins["x"].data_ptr(), ins["w"].data_ptr(), ins["bias"].data_ptr(), out.data_ptr()
    a.n_img, a.Cin, a.Cout, a.H, a.Wd, a.img_stride, a.ch_stride = n_img, Cin, Cout, H, W, kw["img_stride"], kw["ch_stride"]
    a.in_is_f16, a.silu, a.frames, a.frame_stride = int(f16in), int(kw["silu"]), frames, kw.get("frame_stride", 0)
    got = run_guarded(lambda: call(ops, "me_conv_small", C.byref(a)), ins, {"out": out})
    check(got["out"], emu.conv_small(x.float(), wt, bias, **kw), f"guard conv_small {Cin}->{Cout}")


# ------------------------------------------------------------------ me_attn
def attn_case(ops, q, k, v, si, sm, kernel, *, name, mask=None, lse=False, panels=False, q_items=0, **args):
    heads, dh = args["heads"], args["dh"]
    n_kv = k.shape[0] // args["nk"]
    # integer surroundings: kv item indices that exist; modes stay 0 (a stray mode could name a path whose operands are NULL)
    ins = {"seg_item": V(si, int_poison=(0, min(1, n_kv - 1), 0)), "seg_mode": V(sm, int_poison=(0, 0, 0)), "mask": V(mask)}
    if panels:
        hm = lambda t: t.reshape(t.shape[0], heads, dh).permute(1, 0, 2)      # noqa: E731
        ins.update(q=E(hm(q)), k=E(hm(k)), v=E(hm(v)))
    else:
        ins.update(q=E(q), k=E(k), v=E(v))
    rows = args["n_items"] * args["nq"]
    outs = {"out": O((rows, heads * dh))}
    if lse:
        outs["lse"] = O((rows, heads), F32, contiguous=True)
    got = run_guarded(lambda: ops.attention(ins["q"], ins["k"], ins["v"], seg_item=ins["seg_item"], seg_mode=ins["seg_mode"], mask=ins["mask"], out=outs["out"],
                                            lse=outs.get("lse"), q_items=q_items, **args), ins, outs)
    kernel_is(ops, kernel)
    lse_want = torch.empty((rows, heads)) if lse else None
    check(got["out"], emu.attention(q, k, v, seg_item=si, seg_mode=sm, mask=mask, lse=lse_want, q_items=q_items, **args), name)
    if lse:
        check(got["lse"], lse_want, name + " log-sum-exp")


# the kernel forms of the two-segment launch: 16 queries per wave below one whole 256-query block, the wider blocks from there on
PREV_CUR_KERNEL = {(40, False): "attn2_kernel<40,2,4,classic>", (80, False): "attn2_kernel<80,2,4,classic>", (160, False): "attn2_kernel<160,1,4,classic>",
                   (40, True): "attn2_kernel<40,2,8,fold>", (80, True): "attn2_kernel<80,2,8,fold>", (160, True): "attn2_kernel<160,1,4,classic>"}


@pytest.mark.parametrize("dh", [40, 80, 160])
@pytest.mark.parametrize("nq", [1, 100, 300])
@pytest.mark.parametrize("panels", [False, True])
@guards("me_attn")
def test_guard_attention_prev_cur(ops, dh, nq, panels):
    from motioneditor_amd import segments
    B, f, Cc = 2, 3, 8 * dh
    qkv = rnd(B * f * nq, 3 * Cc, seed=1)
    si, sm = segments.prev_cur(B, f, "cpu")
    attn_case(ops, qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], si, sm, PREV_CUR_KERNEL[dh, nq >= 256], name=f"guard attn prev|cur dh={dh} nq={nq}", lse=not panels, panels=panels,
              heads=8, dh=dh, n_items=B * f, nq=nq, nk=nq)


@pytest.mark.parametrize("dh,nq,nk,B,f,kernel", [(40, 100, 77, 4, 2, "attn2_kernel<40,2,4,classic>"), (80, 100, 65, 2, 2, "attn2_kernel<80,2,4,classic>"),
                                                 (160, 1, 77, 2, 3, "attn2_kernel<160,1,4,classic>"), (40, 600, 65, 2, 2, "attn2_kernel<40,2,8,kvres>"),
                                                 (80, 320, 70, 2, 2, "attn2_kernel<80,1,8,kvres>"), (160, 300, 77, 2, 2, "attn2_kernel<160,1,8,kvres>")])
@guards("me_attn")
def test_guard_attention_text_keys(ops, dh, nq, nk, B, f, kernel):
    """One segment of 65 / 77 keys: the last item's last key tile ends exactly where the K and V views end."""
    from motioneditor_amd import segments
    Cc = 8 * dh
    q, kv = rnd(B * f * nq, Cc, seed=1), rnd(B * nk, 2 * Cc, seed=2)
    si, sm = segments.cross_text(B, f, "cpu")
    attn_case(ops, q, kv[:, :Cc], kv[:, Cc:], si, sm, kernel, name=f"guard attn text dh={dh} nq={nq} nk={nk}", lse=True,
              heads=8, dh=dh, n_items=B * f, nq=nq, nk=nk)


@pytest.mark.parametrize("dh,nq,nk,kernel,env", [(40, 520, 520, "attn2_kernel<40,2,16,fold>", None), (40, 300, 100, "attn2_kernel<40,2,8,classic>", None),
                                                 (80, 100, 300, "attn2_kernel<80,2,4,fold>", None), (80, 130, 300, "attn2_kernel<80,1,8,fold>", None),
                                                 (80, 300, 300, "attn2_kernel<80,1,8,fold>", "ME_ATTN_80_QT2"), (80, 130, 100, "attn2_kernel<80,1,8,classic>", None)])
@guards("me_attn")
def test_guard_attention_remaining_forms_of_the_dispatch(ops, dh, nq, nk, kernel, env, monkeypatch):
    """The forms of me_attn's dispatch the cases above do not select, one self-attention segment each, nq and nk off their blocks: 16 waves from 512 queries on
    (the level-0 launch), the 8-wave classic form below 256 keys, the dh = 80 forms below 128 / 256 queries, and the 16-queries-per-wave form that
    ME_ATTN_80_QT2=0 (read per call) keeps for whole 256-query blocks."""
    from motioneditor_amd import segments
    if env:
        monkeypatch.setenv(env, "0")
    Cc = 8 * dh
    q, kv = rnd(2 * nq, Cc, seed=1), rnd(2 * nk, 2 * Cc, seed=2)
    si, sm = segments.self_items(2, "cpu")
    attn_case(ops, q, kv[:, :Cc], kv[:, Cc:], si, sm, kernel, name=f"guard attn dh={dh} nq={nq} nk={nk}", lse=True, heads=8, dh=dh, n_items=2, nq=nq, nk=nk)


@pytest.mark.parametrize("dh,N", [(40, 100), (80, 100), (160, 40)])
@guards("me_attn")
def test_guard_attention_general_dual_with_mask_planes(ops, dh, N):
    from motioneditor_amd import segments
    f, Cc = 2, 8 * dh
    qkv = rnd(4 * f * N, 3 * Cc, seed=1)
    mask = torch.rand(8, N, generator=torch.Generator().manual_seed(7)).half()
    si, sm = segments.edited_spatial(f, "cpu", binary_mask=False)
    attn_case(ops, qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], si, sm, f"attn_kernel<{dh},{1 if dh == 160 else 2},general-dual>", name=f"guard attn general dual dh={dh}", mask=mask,
              heads=8, dh=dh, n_items=4 * f, nq=N, nk=N)


@pytest.mark.parametrize("dh,N", [(40, 100), (80, 144)])
@guards("me_attn")
def test_guard_attention_binary_dual_with_stale_vsum(ops, dh, N):
    """Binary dual segments through the ABI with a NaN-filled vsum scratch (ops.attention allocates it per call): its head, the column sums of V, is written by
    the launch; nothing before or behind the bytes me_attn_vsum_bytes asked for is."""
    from motioneditor_amd import capi, segments
    f, Cc = 2, 8 * dh
    qkv = rnd(4 * f * N, 3 * Cc, seed=1)
    mask = (torch.rand(8, N, generator=torch.Generator().manual_seed(7)) > 0.5).half()
    si, sm = segments.edited_spatial(f, "cpu", binary_mask=True)
    q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    ins = {"q": E(q), "k": E(k), "v": E(v), "seg_item": V(si, int_poison=(0, 1, 0)), "seg_mode": V(sm, int_poison=(0, 0, 0))}
    n_kv = 4 * f
    nb = lib().me_attn_vsum_bytes(n_kv, Cc)
    vsum = torch.empty(nb // 4 + 64, dtype=F32, device="cuda")
    out = O((4 * f * N, Cc))
    a = capi.AttnArgs()
    a.Q, a.K, a.V, a.O = ins["q"].data_ptr(), ins["k"].data_ptr(), ins["v"].data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = ins["q"].stride(0), ins["k"].stride(0), ins["v"].stride(0), out.stride(0)
    a.heads, a.dh, a.n_items, a.nq, a.nk, a.nseg = 8, dh, 4 * f, N, N, si.shape[1]
    a.seg_item, a.seg_mode, a.scale, a.vsum, a.n_kv_items = ins["seg_item"].data_ptr(), ins["seg_mode"].data_ptr(), dh ** -0.5, vsum.data_ptr() + 16, n_kv
    got = run_guarded(lambda: call(ops, "me_attn", C.byref(a)), ins, {"out": out}, before=lambda: vsum.fill_(float("nan")))
    kernel_is(ops, {40: "attn2_kernel<40,2,4,classic>", 80: "attn2_kernel<80,1,8,classic>"}[dh])
    assert bool(torch.isnan(vsum[:4]).all()) and bool(torch.isnan(vsum[4 + nb // 4:]).all()), "me_attn wrote outside the vsum scratch it asked for"
    check(vsum[4:4 + n_kv * Cc].reshape(n_kv, Cc), v.float().reshape(n_kv, N, Cc).sum(1), "guard attn vsum head")
    check(got["out"], emu.attention(q, k, v, seg_item=si, seg_mode=sm, mask=mask, heads=8, dh=dh, n_items=4 * f, nq=N, nk=N), f"guard attn binary dual dh={dh}")


@guards("me_attn")
def test_guard_attention_shared_query_items_and_fixed_offset_fallback(ops):
    from motioneditor_amd import segments
    g = torch.Generator().manual_seed(11)
    dh, nq, f, nb = 40, 100, 3, 2
    Cc = 8 * dh
    q = (torch.randn(f * nq, Cc, generator=g) * 0.7).half()
    kv = (torch.randn(nb * f * nq, 2 * Cc, generator=g) * 0.7).half()
    si, sm = segments.self_items(nb * f, "cpu")
    attn_case(ops, q, kv[:, :Cc], kv[:, Cc:], si, sm, "attn2_kernel<40,2,4,classic>", name="guard attn q_items", q_items=f, heads=8, dh=dh, n_items=nb * f, nq=nq, nk=nq)
    # a key ~ e^35 heavier than the first tile promised: the block is recomputed with the running maximum (test_attention_fixed_offset_overflow_falls_back_...)
    nq, nk, n_items, scale = 96, 640 - 7, 2, dh ** -0.5
    q, k, v = torch.randn(n_items * nq, Cc, generator=g) * 0.5, torch.randn(n_items * nk, Cc, generator=g) * 0.5, torch.randn(n_items * nk, Cc, generator=g)
    for it in range(n_items):
        for h in range(8):
            qs = q[it * nq:(it + 1) * nq, h * dh:(h + 1) * dh]
            d = qs.mean(0)
            d = d / d.norm()
            qs += d * 3.0
            k[it * nk + nk - 70, h * dh:(h + 1) * dh] = d * (35.0 / (3.0 * scale))
    si, sm = segments.self_items(n_items, "cpu")
    ops.attention_fallback_blocks(reset=True)
    attn_case(ops, q.half(), k.half(), v.half(), si, sm, "attn2_kernel<40,2,4,fold>", name="guard attn fallback", heads=8, dh=dh, n_items=n_items, nq=nq, nk=nk)
    assert ops.attention_fallback_blocks() > 0


# ------------------------------------------------------------------ me_tattn
@pytest.mark.parametrize("F,dh,npix,kv_map,parts,qf,q0,qparts", [(7, 40, 5, None, 1, 0, 0, 1), (24, 80, 3, [0, 0, 2, 2], 1, 0, 0, 1), (48, 40, 2, None, 1, 0, 0, 1), (24, 160, 1, None, 1, 0, 0, 1),
                                                              (24, 80, 3, [0, 0, 2, 2], 3, 8, 8, 1), (24, 40, 3, [0, 0, 2, 2], 4, 0, 0, 4)])
@guards("me_tattn")
def test_guard_temporal_attention(ops, F, dh, npix, kv_map, parts, qf, q0, qparts):
    """Both kernels (F <= 32 and 48), an odd frame count, the editor's kv_map, sharded queries over part-major K | V, part-major q and K | V."""
    from motioneditor_amd import capi
    B, Cc = 4, 8 * dh
    q, kv = rnd(B * (qf or F) * npix, Cc, seed=1), rnd(B * F * npix, 2 * Cc, seed=2)
    ins = {"q": E(q), "k": E(kv[:, :Cc]), "v": E(kv[:, Cc:])}
    out = O((q.shape[0], Cc))
    a = capi.TAttnArgs()
    a.Q, a.K, a.V, a.O = ins["q"].data_ptr(), ins["k"].data_ptr(), ins["v"].data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = ins["q"].stride(0), ins["k"].stride(0), ins["v"].stride(0), out.stride(0)
    a.heads, a.dh, a.batch, a.frames, a.npix, a.scale = 8, dh, B, F, npix, dh ** -0.5
    for i, m in enumerate(kv_map or range(B)):
        a.kv_map[i] = m
    a.q_frames, a.q_frame0, a.kv_parts, a.q_parts = qf, q0, parts, qparts
    got = run_guarded(lambda: call(ops, "me_tattn", C.byref(a)), ins, {"out": out})
    want = emu.temporal_attention(q, kv[:, :Cc], kv[:, Cc:], heads=8, dh=dh, batch=B, frames=F, npix=npix, kv_map=kv_map, q_frames=qf, q_frame0=q0, kv_parts=parts, q_parts=qparts)
    check(got["out"], want, f"guard tattn F={F} dh={dh} parts={parts}")


# ------------------------------------------------------------------ norms
def _groupnorm_case(ops, Cc, rows, rpg, silu, **kw):
    x = (rnd(rows, Cc, seed=1) * 2 + 0.7).half()
    gm, bt = (1 + 0.1 * rnd(Cc, seed=2)).half(), (0.1 * rnd(Cc, seed=3)).half()
    ins = {"x": E(x), "gamma": V(gm), "beta": V(bt)}
    out = O((rows, Cc))
    got = run_guarded(lambda: ops.groupnorm(ins["x"], ins["gamma"], ins["beta"], out=out, rows_per_group=rpg, eps=1e-5, silu=silu, **kw), ins, {"out": out}, before=_poison(ops))
    check(got["out"], emu.groupnorm(x, gm, bt, rows_per_group=rpg, eps=1e-5, silu=silu), f"guard groupnorm C={Cc}")


@pytest.mark.parametrize("Cc,rows,rpg,silu", [(320, 4 * 100, 100, True), (640, 96, 8, False), (1280, 64 + 16, 16, True), (2560, 8 * 33, 33, True)])
@guards("me_groupnorm")
def test_guard_groupnorm(ops, Cc, rows, rpg, silu):
    _groupnorm_case(ops, Cc, rows, rpg, silu)


@pytest.mark.parametrize("Cc,rows,rpg,silu", [(640, 4 * 96, 96, True), (320, 2 * 1000, 1000, False)])
@guards("me_groupnorm_stats", "me_groupnorm_apply")
def test_guard_groupnorm_stats_and_apply(ops, Cc, rows, rpg, silu):
    """stats -> reduce hook -> apply: doubling the statistics and the count is the identity."""
    _groupnorm_case(ops, Cc, rows, rpg, silu, reduce=lambda st: st.mul_(2.0), rows_per_group_total=2 * rpg)


@guards("me_groupnorm", "me_groupnorm_bwd", "me_gemm_dw", "me_colsum", "me_layernorm_bwd_params", "me_sumsq_absmax")
def test_guard_scratch_users_after_a_larger_launch(ops):
    """The grow-only reuse a step performs, for the entry points that take scratch from ops._work / ops._gn_scratch: a larger launch first, then the smaller one,
    against the smaller one on NaN-filled scratch -- bitwise.  Exception: ops._gn_scratch is keyed by its size, so the larger me_groupnorm launch fills ANOTHER block
    and only the NaN half of the protocol says something about me_groupnorm; the other five share one grow-only block per purpose."""
    g = torch.Generator().manual_seed(31)

    def gn(rows, rpg, Cc):
        x, gm, bt = E((rnd(rows, Cc, seed=rows) * 2 + 0.7).half()), V((1 + 0.1 * rnd(Cc, seed=2)).half()), V((0.1 * rnd(Cc, seed=3)).half())
        return lambda: ops.groupnorm(x, gm, bt, rows_per_group=rpg, eps=1e-5, silu=True)

    def gnb(rows, rpg, Cc):
        x, gm, bt, dy = E((rnd(rows, Cc, seed=rows) * 1.5 + 0.5).half()), V((1 + 0.2 * rnd(Cc, seed=2)).half()), V((0.2 * rnd(Cc, seed=3)).half()), E(torch.randn(rows, Cc, generator=g))
        return lambda: ops.groupnorm_bwd(x, gm, bt, dy, rows_per_group=rpg, eps=1e-5, silu=True)

    def dw(M, N, K):
        x, dy, base = E(rnd(M, K, seed=M)), E(torch.randn(M, N, generator=g)), _acc0((N, 1, K)).cuda()
        return lambda: ops.gemm_dw(dy, x, dst=base.clone(), taps=1, K=K, M=M)

    def cs(M, N):
        dy, base = E(torch.randn(M, N, generator=g)), _acc0((N,)).cuda()
        return lambda: ops.colsum_grad(dy, dst=base.clone())

    def lnp(M, Cc):
        x, dy, g0, b0 = E((rnd(M, Cc, seed=M) * 2 + 0.3).half()), E(torch.randn(M, Cc, generator=g)), _acc0((Cc,), 1).cuda(), _acc0((Cc,), 2).cuda()

        def run():
            dg, db = g0.clone(), b0.clone()
            ops.layernorm_bwd_params(x, dy, dgamma=dg, dbeta=db, eps=1e-5)
            return {"dgamma": dg, "dbeta": db}
        return run

    def ssq(n):
        x = V(torch.randn(n, generator=g) * 3)
        return lambda: ops.sumsq_absmax(x).clone()

    for small, large in ((gn(2 * 33, 33, 320), gn(8 * 100, 100, 640)), (gnb(2 * 50, 50, 320), gnb(3 * 700, 700, 640)), (dw(300, 320, 192), dw(3000, 640, 640)),
                         (cs(300, 320), cs(5000, 1280)), (lnp(333, 320), lnp(5000, 1280)), (ssq(1003), ssq(3_000_001))):
        scratch_independent(small, _poison(ops), run_larger=large)


@pytest.mark.parametrize("Cc,rows", [(320, 1001), (320, 4096 * 2 + 5), (640, 77), (1280, 131)])     # >= 4096 rows of 320: the half-wave-per-row kernel; odd row tails
@guards("me_layernorm")
def test_guard_layernorm(ops, Cc, rows):
    from motioneditor_amd import capi
    x = (rnd(rows, Cc, seed=1) * 3 - 0.4).half()
    gm, bt = (1 + 0.1 * rnd(Cc, seed=2)).half(), (0.1 * rnd(Cc, seed=3)).half()
    ins = {"x": E(x), "gamma": V(gm), "beta": V(bt)}
    out = O((rows, Cc))
    a = capi.LayerNormArgs()
    a.X, a.Y, a.gamma, a.beta = ins["x"].data_ptr(), out.data_ptr(), ins["gamma"].data_ptr(), ins["beta"].data_ptr()
    a.rows, a.C, a.ldx, a.ldy, a.eps = rows, Cc, ins["x"].stride(0), out.stride(0), 1e-5
    got = run_guarded(lambda: call(ops, "me_layernorm", C.byref(a)), ins, {"out": out})
    check(got["out"], emu.layernorm(x, gm, bt), f"guard layernorm C={Cc} rows={rows}")


@pytest.mark.parametrize("Cc,rows", [(640, 1001), (1280, 77), (64, 33)])      # parts of 320 columns; one part over a row that is not a multiple of 320
@guards("me_ln_stats")
def test_guard_ln_stats(ops, Cc, rows):
    x = (rnd(rows, Cc, seed=1) * 3 - 0.4).half()
    P = Cc // 320 if Cc % 320 == 0 else 1
    xg, st = E(x), O((P, rows, 2), F32, contiguous=True)
    got = run_guarded(lambda: call(ops, "me_ln_stats", xg.data_ptr(), xg.stride(0), rows, Cc, st.data_ptr(), st.stride(0)), {"x": xg}, {"st": st})
    kernel_is(ops, "ln_stats")
    xf = x.float().reshape(rows, P, Cc // P)
    check(got["st"][:, :, 0].t(), xf.sum(-1), "guard ln_stats sum")
    check(got["st"][:, :, 1].t(), (xf * xf).sum(-1), "guard ln_stats sumsq")


@pytest.mark.parametrize("rows,cols", [(33, 72), (130, 1024), (9, 8192)])
@guards("me_softmax_rows")
def test_guard_softmax_rows(ops, rows, cols):
    x = rnd(rows, cols, seed=1, scale=0.5)       # flat rows: the bound of check() is relative to the MEAN probability, the fp16 rounding to the largest one
    xg, out = E(x), O((rows, cols))
    got = run_guarded(lambda: ops.softmax_rows(xg, out=out), {"x": xg}, {"out": out})
    check(got["out"], emu.softmax_rows(x), f"guard softmax {rows}x{cols}")
    got = run_guarded(lambda: ops.softmax_rows(xg, out=xg), {"x": xg}, {}, inout=["x"])      # in place
    check(got["x"], emu.softmax_rows(x), "guard softmax in place")


# ------------------------------------------------------------------ element-wise and layout
@guards("me_axpy_rows", "me_copy_rows", "me_copy_blocks")
def test_guard_axpy_and_copies(ops):
    x, a = rnd(100, 648, seed=1), rnd(100, 648, seed=2)
    ins = {"x": E(x), "a": E(a)}
    y = O((100, 648))
    got = run_guarded(lambda: ops.axpy_rows(y, ins["x"], ins["a"], 0.5), ins, {"y": y})
    check(got["y"], x.float() + 0.5 * a.float(), "guard axpy_rows")
    got = run_guarded(lambda: ops.axpy_rows(ins["x"], ins["x"], ins["a"], 0.5), ins, {}, inout=["x"])       # y is x
    check(got["x"], x.float() + 0.5 * a.float(), "guard axpy_rows in place")
    src = E(x)
    got = run_guarded(lambda: ops.copy_rows(y, src), {"x": src}, {"y": y})
    assert torch.equal(got["y"].cpu(), x)
    R, BF, Ns, W = 4, 6, 16, 48
    xb = rnd(BF * R * Ns, W, seed=4)
    src, yb = E(xb), O((R * BF * Ns, W))
    got = run_guarded(lambda: ops.copy_blocks(yb, src, R, BF, Ns, ys0=BF * Ns, ys1=Ns, xs0=Ns, xs1=R * Ns), {"x": src}, {"y": yb})
    assert torch.equal(got["y"].cpu(), xb.reshape(BF, R, Ns, W).permute(1, 0, 2, 3).reshape(-1, W))


def _flat_case(ops, sym, n, want):
    x = torch.cat([rnd(n - 2, seed=6, scale=2.0), torch.tensor([-11.0, 11.0]).half()])
    xg, y = V(x), O((n,), contiguous=True)
    got = run_guarded(lambda: call(ops, sym, y.data_ptr(), xg.data_ptr(), n), {"x": xg}, {"y": y})
    check(got["y"], want(x), f"guard {sym} n={n}")


@pytest.mark.parametrize("n", [5, 8 * 1001 + 3, 300 * 640])
@guards("me_silu", "me_relu")
def test_guard_silu_relu(ops, n):
    """n % 8 != 0: the scalar tail of unary_kernel behind the last whole 16-byte vector."""
    _flat_case(ops, "me_silu", n, emu.silu)
    _flat_case(ops, "me_relu", n, emu.relu)


@pytest.mark.parametrize("n", [3, 8 * 1000 + 5, 77 * 3072])
@guards("me_quick_gelu")
def test_guard_quick_gelu(ops, n):
    """n % 8 != 0: the scalar tail loop behind the last whole 16-byte vector."""
    _flat_case(ops, "me_quick_gelu", n, lambda t: emu_clip.quick_gelu(t.float()))
    kernel_is(ops, "quick_gelu_kernel")


@pytest.mark.parametrize("n_seq,seq,vocab,Cc", [(3, 77, 1000, 768), (1, 5, 300, 64)])
@guards("me_embed_rows")
def test_guard_embed_rows(ops, n_seq, seq, vocab, Cc):
    tok, pos = rnd(vocab, Cc, seed=1, scale=0.05), rnd(seq + 3, Cc, seed=2, scale=0.05)
    ids = torch.randint(0, vocab, (n_seq * seq,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    ids[0], ids[-1] = vocab - 1, 0
    ins = {"tok": V(tok, row_guard=8, col_guard=Cc), "pos": V(pos, row_guard=8, col_guard=Cc), "ids": V(ids, int_poison=(0, 1, vocab - 1))}
    out = O((n_seq * seq, Cc), contiguous=True)
    got = run_guarded(lambda: call(ops, "me_embed_rows", out.data_ptr(), ins["tok"].data_ptr(), ins["pos"].data_ptr(), ins["ids"].data_ptr(), n_seq * seq, seq, Cc, vocab), ins, {"out": out})
    kernel_is(ops, "embed_rows_kernel")
    assert torch.equal(got["out"].cpu(), emu_clip.embed_rows(tok, pos, ids, seq))


@pytest.mark.parametrize("n_seq,heads,nq", [(3, 2, 16), (2, 12, 77), (2, 3, 128)])
@guards("me_attn_causal")
def test_guard_attention_causal(ops, n_seq, heads, nq):
    Cc = heads * 64
    qkv = rnd(n_seq * nq, 3 * Cc, seed=4)
    qkv[:, :2 * Cc] *= 3.0
    ins = {"q": E(qkv[:, :Cc]), "k": E(qkv[:, Cc:2 * Cc]), "v": E(qkv[:, 2 * Cc:])}
    out = O((n_seq * nq, Cc))
    got = run_guarded(lambda: call(ops, "me_attn_causal", out.data_ptr(), out.stride(0), ins["q"].data_ptr(), ins["q"].stride(0), ins["k"].data_ptr(), ins["k"].stride(0),
                                   ins["v"].data_ptr(), ins["v"].stride(0), n_seq, heads, 64, nq, 64 ** -0.5), ins, {"out": out})
    kernel_is(ops, "attn_causal_kernel")
    check(got["out"], emu_clip.attention_causal(qkv[:, :Cc].float(), qkv[:, Cc:2 * Cc].float(), qkv[:, 2 * Cc:].float(), heads=heads, dh=64, n_seq=n_seq, nq=nq), f"guard attn_causal nq={nq}")


@guards("me_timestep_embed", "me_timestep_embed_dev", "me_cfg_ddim", "me_cfg_ddim_dev", "me_gaussian_sample")
def test_guard_step_scalars_and_sampling(ops):
    params = V(torch.tensor([981.0, 7.5, 1.01, -0.07]))       # {t, guidance, ca, cb}: the device-resident scalars of a captured step
    out = O((3, 320), contiguous=True)      # (no leading dimension in the ABI)
    got = run_guarded(lambda: call(ops, "me_timestep_embed", out.data_ptr(), 3, 320, 981.0), {}, {"out": out})
    check(got["out"], emu.timestep_embed(3, 320, 981.0, "cpu"), "guard timestep_embed")
    got = run_guarded(lambda: call(ops, "me_timestep_embed_dev", out.data_ptr(), 3, 320, params.data_ptr()), {"params": params}, {"out": out})
    check(got["out"], emu.timestep_embed(3, 320, 981.0, "cpu"), "guard timestep_embed_dev")
    lat, eps = torch.randn(2, 4, 3, 5, 7, generator=torch.Generator().manual_seed(3)), rnd(4 * 3 * 35, 4, seed=4)
    ins = {"lat": V(lat), "eps": E(eps), "params": params}
    o = O(lat.shape, F32)
    want = emu.cfg_ddim(lat, eps, guidance=7.5, ca=1.01, cb=-0.07)
    got = run_guarded(lambda: call(ops, "me_cfg_ddim", o.data_ptr(), ins["lat"].data_ptr(), ins["eps"].data_ptr(), ins["eps"].stride(0), 2, 4, 3, 35, 7.5, 1.01, -0.07), ins, {"out": o})
    check(got["out"], want, "guard cfg_ddim")
    got = run_guarded(lambda: call(ops, "me_cfg_ddim_dev", o.data_ptr(), ins["lat"].data_ptr(), ins["eps"].data_ptr(), ins["eps"].stride(0), 2, 4, 3, 35, params.data_ptr()), ins, {"out": o})
    check(got["out"], want, "guard cfg_ddim_dev")
    n_img, npix = 3, 35
    mom, noise = rnd(n_img * npix, 8, seed=5), torch.randn(n_img, 4, npix, generator=torch.Generator().manual_seed(6))
    ins = {"moments": E(mom), "noise": V(noise)}
    o = O((n_img, 4, npix), F32, contiguous=True)
    got = run_guarded(lambda: call(ops, "me_gaussian_sample", o.data_ptr(), ins["moments"].data_ptr(), ins["moments"].stride(0), ins["noise"].data_ptr(), n_img, npix, 0.5), ins, {"out": o})
    check(got["out"], emu.gaussian_sample(mom, noise, n_img, npix, 0.5), "guard gaussian_sample")


@guards("me_nchw_to_rows", "me_rows_to_nchw")
def test_guard_layout_conversions(ops):
    """4-D and the 5-D pair (one launch per batch entry with the frame / channel strides of [B, C, f, h, w])."""
    n_img, Cc, npix = 3, 8, 35
    x = torch.randn(n_img, Cc, npix, generator=torch.Generator().manual_seed(5))
    xg, rows = V(x), O((n_img * npix, Cc))
    got = run_guarded(lambda: call(ops, "me_nchw_to_rows", rows.data_ptr(), rows.stride(0), xg.data_ptr(), Cc * npix, npix, n_img, Cc, npix), {"x": xg}, {"rows": rows})
    check(got["rows"], emu.nchw_to_rows(x, n_img, Cc, npix, Cc * npix, npix), "guard nchw_to_rows")
    rg, back = E(x.permute(0, 2, 1).reshape(n_img * npix, Cc).half()), O((n_img, Cc, npix), F32, contiguous=True)
    got = run_guarded(lambda: call(ops, "me_rows_to_nchw", back.data_ptr(), Cc * npix, npix, rg.data_ptr(), rg.stride(0), n_img, Cc, npix), {"rows": rg}, {"x": back})
    check(got["x"], x.half().float(), "guard rows_to_nchw")
    B, f, h, w = 2, 3, 4, 5
    t5 = torch.randn(B, Cc, f, h, w, generator=torch.Generator().manual_seed(6))
    x5, rows5 = V(t5), O((B * f * h * w, Cc))

    def to_rows():
        for b in range(B):
            call(ops, "me_nchw_to_rows", rows5[b * f * h * w:].data_ptr(), rows5.stride(0), x5[b].data_ptr(), h * w, f * h * w, f, Cc, h * w)
    got = run_guarded(to_rows, {"x": x5}, {"rows": rows5})
    check(got["rows"], emu.nchw5_to_rows(t5), "guard nchw5_to_rows")
    rg5, back5 = E(emu.nchw5_to_rows(t5).half()), O((B, Cc, f, h, w), F32)

    def to_nchw():
        for b in range(B):
            call(ops, "me_rows_to_nchw", back5[b].data_ptr(), h * w, f * h * w, rg5[b * f * h * w:].data_ptr(), rg5.stride(0), f, Cc, h * w)
    got = run_guarded(to_nchw, {"rows": rg5}, {"x": back5})
    check(got["x"], t5.half().float(), "guard rows_to_nchw5")


# ------------------------------------------------------------------ backward and training
@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("mode", ["dense", "dense_n4", "conv", "conv_s2", "conv_ups", "tconv", "geglu_w"])
@guards("me_grad_acc", "me_cast_rows_f16")
def test_guard_gemm_dx(ops, mode, store):
    """The modes of test_gemm_dx_matches_the_vjp_of_the_forward_emulation through the wrapper.  Under guard are the operands the wrapper passes on as they are: dy
    into me_cast_rows_f16 and dst (in-out, or store: written without being read) into me_grad_acc, in every mode's row count and pooling.  The me_gemm in between
    runs on the wrapper's own contiguous temporaries (the fp16 copy of dy, the transposed weights it builds from the guarded w, its product), so it is NOT guarded
    here: its gather forms, the zero-stuffed one included, are test_guard_gemm_conv3x3 / _tconv / _dense."""
    g = torch.Generator().manual_seed(5)
    conv = tconv = None
    if mode in ("dense", "geglu_w"):
        M, N, K, taps, xr = 384, 320 if mode == "dense" else 640, 192, 1, 384
    elif mode == "dense_n4":
        M, N, K, taps, xr = 256, 4, 320, 1, 256
    elif mode == "conv":
        M, N, K, taps, xr, conv = 2 * 16 * 16, 128, 64, 9, 2 * 16 * 16, (16, 16, 16, 16, 1, 0)
    elif mode == "conv_s2":
        M, N, K, taps, xr, conv = 2 * 8 * 8, 128, 64, 9, 2 * 16 * 16, (16, 16, 8, 8, 2, 0)
    elif mode == "conv_ups":
        M, N, K, taps, xr, conv = 2 * 16 * 16, 128, 64, 9, 2 * 8 * 8, (8, 8, 16, 16, 1, 1)
    else:
        M, N, K, taps, xr, tconv = 2 * 8 * 12, 128, 64, 3, 2 * 8 * 12, (8, 12, 8)
    w = (torch.randn(N, taps, K, generator=g) * (taps * K) ** -0.5).half()
    dy = torch.randn(M, N, generator=g)
    base = _acc0((xr, K))
    want = torch.zeros_like(base) if store else base.clone()
    emu.gemm_dx(dy.half().float(), w, dst=want, M=M, conv=conv, tconv=tconv)
    ins = {"dy": E(dy), "w": V(w, row_guard=128 * taps, col_guard=K), "dst": E(base)}

    def launch():
        ops.invalidate_transposed()
        ops.gemm_dx(ins["dy"], ins["w"], dst=ins["dst"], M=M, conv=conv, tconv=tconv, store=store)
    got = run_guarded(launch, ins, {}, inout=["dst"])
    ops.invalidate_transposed()
    check(got["dst"], want, f"guard gemm_dx {mode} store={store}")


@pytest.mark.parametrize("mode", ["dense", "tconv", "dense_f16"])
@guards("me_gemm_dw", "me_colsum")
def test_guard_gemm_dw_and_colsum(ops, mode):
    g = torch.Generator().manual_seed(12)
    M, N, K, taps, tconv = (300, 320, 192, 1, None) if mode != "tconv" else (2 * 16 * 12, 128, 64, 3, (16, 12, 8))
    x, dy = torch.randn(M, K, generator=g).half(), torch.randn(M, N, generator=g)
    dyc = dy.half() if mode == "dense_f16" else dy
    base, b0 = _acc0((N, taps, K)), _acc0((N,))
    ins = {"dy": E(dyc), "x": E(x), "dst": V(base), "bias_grad": V(b0)}
    got = run_guarded(lambda: ops.gemm_dw(ins["dy"], ins["x"], dst=ins["dst"], taps=taps, K=K, M=M, tconv=tconv), ins, {}, inout=["dst"], before=_poison(ops))
    kernel_is(ops, "gemm_dw_kernel")
    want = emu.gemm_dw(dy.half().float(), x, dst=base.clone(), taps=taps, K=K, M=M, tconv=tconv)
    check(got["dst"].cpu() - base, want - base, f"guard gemm_dw {mode}")
    got = run_guarded(lambda: ops.colsum_grad(ins["dy"], dst=ins["bias_grad"]), ins, {}, inout=["bias_grad"], before=_poison(ops))
    check(got["bias_grad"].cpu() - b0, emu.colsum_grad(dyc, dst=b0.clone()) - b0, f"guard colsum {mode}")


@guards("me_geglu_bwd", "me_relu_bwd", "me_softmax_bwd_rows", "me_layernorm_bwd", "me_layernorm_bwd_params")
def test_guard_rowwise_backward_kernels(ops):
    g = torch.Generator().manual_seed(6)
    p = lambda t: (t.data_ptr(), t.stride(0))      # noqa: E731
    M, N = 301, 640
    pre, dy = (torch.randn(M, N, generator=g) * 1.5).half(), torch.randn(M, N // 2, generator=g)
    ins, out = {"pre": E(pre), "dy": E(dy)}, O((M, N))
    got = run_guarded(lambda: call(ops, "me_geglu_bwd", *p(out), *p(ins["pre"]), *p(ins["dy"]), M, N), ins, {"out": out})
    check(got["out"], emu.geglu_bwd(pre, dy), "guard geglu_bwd")
    rows, Cc = 333, 320
    fwd, dy = torch.randn(rows, Cc, generator=g).half(), torch.randn(rows, Cc, generator=g)
    ins, dx = {"dy": E(dy), "out": E(fwd)}, O((rows, Cc), F32)
    got = run_guarded(lambda: call(ops, "me_relu_bwd", *p(dx), *p(ins["dy"]), *p(ins["out"]), rows, Cc), ins, {"dx": dx})
    assert torch.equal(got["dx"].cpu(), emu.relu_bwd(dy, fwd))
    rows, cols = 33, 72
    P, dP = emu.softmax_rows(rnd(rows, cols, seed=1)).half(), rnd(rows, cols, seed=2)
    ins, dS = {"P": E(P), "dP": E(dP)}, O((rows, cols))
    got = run_guarded(lambda: call(ops, "me_softmax_bwd_rows", *p(dS), *p(ins["P"]), *p(ins["dP"]), rows, cols, 0.25), ins, {"dS": dS})
    Pf, dPf = P.float(), dP.float()
    check(got["dS"], Pf * (dPf - (Pf * dPf).sum(-1, keepdim=True)) * 0.25, "guard softmax_bwd_rows")
    for Cc, rows in ((320, 257), (1280, 33)):
        x, gm, dy = (torch.randn(rows, Cc, generator=g) * 2 + 0.3).half(), (1 + 0.2 * torch.randn(Cc, generator=g)).half(), torch.randn(rows, Cc, generator=g)
        ins, dx = {"x": E(x), "gamma": V(gm), "dy": E(dy)}, O((rows, Cc), F32)
        got = run_guarded(lambda: call(ops, "me_layernorm_bwd", *p(dx), *p(ins["x"]), ins["gamma"].data_ptr(), *p(ins["dy"]), rows, Cc, 1e-5), ins, {"dx": dx})
        check(got["dx"], emu.layernorm_bwd(x, gm, dy, eps=1e-5), f"guard layernorm_bwd C={Cc}")
        g0, b0 = _acc0((Cc,), 1), _acc0((Cc,), 2)
        ins = {"x": ins["x"], "dy": ins["dy"], "dgamma": V(g0), "dbeta": V(b0)}
        got = run_guarded(lambda: ops.layernorm_bwd_params(ins["x"], ins["dy"], dgamma=ins["dgamma"], dbeta=ins["dbeta"], eps=1e-5), ins, {}, inout=["dgamma", "dbeta"], before=_poison(ops))
        wg, wb = g0.clone(), b0.clone()
        emu.layernorm_bwd_params(x, dy, dgamma=wg, dbeta=wb, eps=1e-5)
        check(got["dgamma"].cpu() - g0, wg - g0, f"guard layernorm d gamma C={Cc}")
        check(got["dbeta"].cpu() - b0, wb - b0, f"guard layernorm d beta C={Cc}")


@pytest.mark.parametrize("Cc,rpg,nsg,silu", [(320, 96, 2, True), (640, 50, 3, False), (2560, 70, 1, False)])
@guards("me_groupnorm_bwd")
def test_guard_groupnorm_bwd(ops, Cc, rpg, nsg, silu):
    g = torch.Generator().manual_seed(8)
    rows = nsg * rpg
    x, gm, bt = (torch.randn(rows, Cc, generator=g) * 1.5 + 0.5).half(), (1 + 0.2 * torch.randn(Cc, generator=g)).half(), (0.2 * torch.randn(Cc, generator=g)).half()
    dy = torch.randn(rows, Cc, generator=g)
    ins, dx = {"x": E(x), "gamma": V(gm), "beta": V(bt), "dy": E(dy)}, O((rows, Cc), F32)
    scratch = ops._work(lib().me_groupnorm_bwd_scratch_bytes(rows, rpg, 32), "cuda", "gnbwd")
    got = run_guarded(lambda: call(ops, "me_groupnorm_bwd", dx.data_ptr(), dx.stride(0), ins["x"].data_ptr(), ins["x"].stride(0), ins["gamma"].data_ptr(), ins["beta"].data_ptr(),
                                   ins["dy"].data_ptr(), ins["dy"].stride(0), rows, rpg, Cc, 32, 1e-5, int(silu), scratch.data_ptr()), ins, {"dx": dx}, before=_poison(ops))
    check(got["dx"], emu.groupnorm_bwd(x, gm, bt, dy, rows_per_group=rpg, eps=1e-5, silu=silu), f"guard groupnorm_bwd C={Cc}")


@pytest.mark.parametrize("F,dh,npix", [(7, 40, 4), (24, 80, 3), (48, 160, 1)])      # F <= 32: the lane-parallel kernel; 48: the first version
@guards("me_tattn_bwd")
def test_guard_temporal_attention_bwd(ops, F, dh, npix):
    g = torch.Generator().manual_seed(9)
    B, Cc = 2, 8 * dh
    rows = B * F * npix
    qkv, dout = (torch.randn(rows, 3 * Cc, generator=g) * 0.7).half(), torch.randn(rows, Cc, generator=g)
    ins = {"q": E(qkv[:, :Cc]), "k": E(qkv[:, Cc:2 * Cc]), "v": E(qkv[:, 2 * Cc:]), "dout": E(dout)}
    outs = {n: O((rows, Cc), F32) for n in ("dq", "dk", "dv")}
    p = lambda t: (t.data_ptr(), t.stride(0))      # noqa: E731
    got = run_guarded(lambda: call(ops, "me_tattn_bwd", *p(outs["dq"]), *p(outs["dk"]), *p(outs["dv"]), *p(ins["q"]), *p(ins["k"]), *p(ins["v"]), *p(ins["dout"]), B, F, npix, 8, dh,
                                   dh ** -0.5), ins, outs)
    want = emu.temporal_attention_bwd(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], None, dout, heads=8, dh=dh, batch=B, frames=F, npix=npix)
    for n, wnt in zip(("dq", "dk", "dv"), want):
        check(got[n], wnt, f"guard tattn_bwd {n} F={F} dh={dh}")


@pytest.mark.parametrize("kind,dh,nq,nk,f", [("pc", 40, 100, 100, 3), ("cross", 80, 100, 77, 3), ("self", 160, 40, 40, 2)])
@guards("me_attn", "me_attn_bwd")
def test_guard_attention_bwd(ops, kind, dh, nq, nk, f):
    """me_attn_bwd on the log-sum-exp the guarded forward stashed; dq, dk, dv are in-out (+=) views, restored before every launch.  Not under guard: the segment
    tables (the wrapper derives its inverse tables from device tables that segments.py built) and the `delta` scratch the wrapper allocates per call."""
    from test_kernels_gpu import _attn_case
    g = torch.Generator().manual_seed(10)
    Cc = 8 * dh
    si, sm, n_items, n_kv = _attn_case(kind, f)
    q, k = (torch.randn(n_items * nq, Cc, generator=g) * 0.7).half(), (torch.randn(n_kv * nk, Cc, generator=g) * 0.7).half()
    v, dout = torch.randn(n_kv * nk, Cc, generator=g).half(), torch.randn(n_items * nq, Cc, generator=g)
    args = dict(heads=8, dh=dh, n_items=n_items, nq=nq, nk=nk)
    w0 = (_acc0((n_items * nq, Cc), 1), _acc0((n_kv * nk, Cc), 2), _acc0((n_kv * nk, Cc), 3))
    sic, smc = _attn_case(kind, f, "cuda")[:2]       # (tables built by segments.py on the device: attention_bwd derives the inverse table from them)
    ins = {"q": E(q), "k": E(k), "v": E(v)}
    fo = {"out": O((n_items * nq, Cc)), "lse": O((n_items * nq, 8), F32, contiguous=True)}
    fwd = run_guarded(lambda: ops.attention(ins["q"], ins["k"], ins["v"], seg_item=sic, seg_mode=smc, out=fo["out"], lse=fo["lse"], **args), ins, fo)
    ins.update(out=E(fwd["out"]), lse=V(fwd["lse"]), dout=E(dout), dq=E(w0[0]), dk=E(w0[1]), dv=E(w0[2]))
    got = run_guarded(lambda: ops.attention_bwd(ins["q"], ins["k"], ins["v"], ins["out"], ins["dout"], dq=ins["dq"], dk=ins["dk"], dv=ins["dv"], lse=ins["lse"], seg_item=sic, seg_mode=smc,
                                                **args), ins, {}, inout=["dq", "dk", "dv"])
    kernel_is(ops, f"attn_bwd_dkv_kernel<{dh},{1 if dh == 160 else 2}>+attn_bwd_dq_kernel")      # keys per block = 64 * NKT: 2 for dh 40 / 80, 1 for dh 160
    want = [t.clone() for t in w0]
    emu.attention_bwd(q, k, v, None, dout, dq=want[0], dk=want[1], dv=want[2], seg_item=si, seg_mode=sm, **args)
    for n, b, z in zip(("dq", "dk", "dv"), want, w0):
        check(got[n].cpu() - z, b - z, f"guard attention_bwd {n} {kind} dh={dh}")


@guards("me_grad_acc", "me_sumsq_absmax", "me_adamw", "me_cast_f16", "me_cast_rows_f16", "me_mse_seed")
def test_guard_training_kernels(ops):
    g = torch.Generator().manual_seed(14)
    rows, cols = 300, 64
    dst0, src = _acc0((rows, cols)), torch.randn(rows + 5, cols + 8, generator=g)
    for s_, name in ((src, "fp32"), (src.half(), "fp16")):      # plain and strided: both operands are views with a leading dimension
        ins = {"dst": E(dst0), "src": E(s_)}
        got = run_guarded(lambda: ops.grad_acc(ins["dst"], ins["src"][:, :cols], 0.5), ins, {}, inout=["dst"])
        check(got["dst"], emu.grad_acc(dst0.clone(), s_[:, :cols], 0.5), f"guard grad_acc {name}")
    n_img, H, W = 3, 6, 10
    big, d0 = torch.randn(n_img * 4 * H * W, cols, generator=g).half(), _acc0((n_img * H * W, cols))
    ins = {"dst": E(d0), "src": E(big)}
    got = run_guarded(lambda: ops.grad_acc(ins["dst"], ins["src"], 1.0, pool=(H, W)), ins, {}, inout=["dst"])
    check(got["dst"], emu.grad_acc(d0.clone(), big, 1.0, pool=(H, W)), "guard grad_acc pooled")
    flat, add = _acc0((77 * 768,)), _acc0((77 * 768,), 5)
    ins = {"dst": V(flat), "src": V(add)}
    got = run_guarded(lambda: ops.grad_acc(ins["dst"], ins["src"], 2.0), ins, {}, inout=["dst"])
    check(got["dst"], flat + 2.0 * add, "guard grad_acc 1-D")
    # sum of squares / absolute maximum of a flat bucket, then the optimiser step on it
    n = 10_003 * 4
    gr = torch.randn(n, generator=g) * 3
    gr[n // 2] = -40.0
    gv, ss = V(gr), O((2,), F32)
    got = run_guarded(lambda: ops.sumsq_absmax(gv, out=ss), {"g": gv}, {"ss": ss}, before=_poison(ops))
    check(got["ss"], torch.tensor([float((gr.double() ** 2).sum()), 40.0]), "guard sumsq_absmax")
    assert float(got["ss"][1]) == 40.0
    p0 = torch.randn(n, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ref.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_([ref], 1.0)
    opt.step()
    ins = {"p": V(p0), "m": V(torch.zeros(n)), "v": V(torch.zeros(n)), "g": V(gr * 256.0)}
    gn = ops.sumsq_absmax(ins["g"]).clone()
    got = run_guarded(lambda: ops.adamw(ins["p"], ins["m"], ins["v"], ins["g"], lr=1e-3, weight_decay=1e-2, step=1, gnorm_sq=gn, max_grad_norm=1.0, grad_scale=1.0 / 256.0), ins, {},
                      inout=["p", "m", "v"])
    check(got["p"], ref.detach(), "guard adamw")
    x = torch.randn(1003 * 8, generator=g) * 10
    xv, o16 = V(x), O((x.numel(),), contiguous=True)
    got = run_guarded(lambda: ops.cast_f16(o16, xv), {"x": xv}, {"out": o16})
    assert torch.equal(got["out"].cpu(), x.half())
    wide = torch.randn(50, 20, generator=g)
    wv, o = E(wide), O((50, 24))
    got = run_guarded(lambda: call(ops, "me_cast_rows_f16", o.data_ptr(), o.stride(0), wv.data_ptr(), wv.stride(0), 50, 20, 24), {"x": wv}, {"out": o})
    assert torch.equal(got["out"][:, :20].cpu(), wide.half()) and float(got["out"][:, 20:].abs().max()) == 0.0
    nb, Cc, f, h, w = 1, 4, 3, 4, 5
    eu, ec = torch.randn(nb * f * h * w, 8, generator=g).half(), torch.randn(nb * f * h * w, 8, generator=g).half()
    xl, tg = torch.randn(nb, Cc, f, h, w, generator=g), torch.randn(nb, Cc, f, h, w, generator=g)
    ins = {"eps_u": E(eu), "eps_c": E(ec), "x": V(xl), "target": V(tg)}
    outs = {"diff": O(tg.shape, F32), "d_eps": O((nb * f * h * w, Cc), F32)}
    got = run_guarded(lambda: call(ops, "me_mse_seed", outs["diff"].data_ptr(), outs["d_eps"].data_ptr(), outs["d_eps"].stride(0), ins["eps_u"].data_ptr(), ins["eps_u"].stride(0),
                                   ins["eps_c"].data_ptr(), ins["eps_c"].stride(0), ins["x"].data_ptr(), ins["target"].data_ptr(), nb, Cc, f, h * w, 7.5, 1.01, -0.2, 0.3), ins, outs)
    d0, r0 = emu.mse_seed(eu, tg, eps_c=ec, x=xl, guidance=7.5, ca=1.01, cb=-0.2, coef=0.3)
    check(got["diff"], d0, "guard mse_seed diff")
    check(got["d_eps"], r0, "guard mse_seed seed rows")


@guards("me_refresh_weights")
def test_guard_refresh_weights_touches_only_the_trained_row_ranges(ops):
    """The table's entries are row ranges INSIDE packed tensors: q's rows of a packed q | k | v weight are refreshed from their fp32 master, the k | v rows after them
    (and the rows of another layer before them) are the guard and must keep their bits -- this is what keeps k | v frozen while q trains.  A LayerNorm-fold entry
    also writes its colsum / cvec ranges inside longer vectors."""
    g = torch.Generator().manual_seed(19)
    K, rows = 320, 320
    packed = rnd(4 * rows, K, seed=1)                       # [another layer | q | k | v]
    master = torch.randn(rows, K, generator=g) * K ** -0.5
    gamma, beta, bias = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(rows, generator=g)
    cs0, cv0 = _acc0((4 * rows,), 3), _acc0((4 * rows,), 4)
    ins = {"packed": V(packed), "folded": V(packed), "master": E(master), "gamma": V(gamma), "beta": V(beta), "bias": V(bias), "colsum": V(cs0), "cvec": V(cv0)}
    sl = slice(rows, 2 * rows)
    table = ops.refresh_table([(ins["master"], ins["packed"][sl], None, None, None, None, None),
                               (ins["master"], ins["folded"][sl], ins["gamma"], ins["beta"], ins["bias"], ins["colsum"][sl], ins["cvec"][sl])])
    got = run_guarded(lambda: ops.refresh_weights(table), ins, {}, inout=["packed", "folded", "colsum", "cvec"])
    keep = torch.ones(4 * rows, dtype=torch.bool)
    keep[sl] = False
    for name in ("packed", "folded"):
        assert torch.equal(got[name].cpu()[keep], packed[keep]), f"{name}: rows outside the trained range were rewritten"
    assert torch.equal(got["packed"].cpu()[sl], master.half())
    wq = (master * gamma[None, :]).half()
    assert torch.equal(got["folded"].cpu()[sl], wq)
    for name, before, want in (("colsum", cs0, wq.float().sum(1)), ("cvec", cv0, master @ beta + bias)):
        assert torch.equal(got[name].cpu()[keep], before[keep]), f"{name}: elements outside the trained range were rewritten"
        check(got[name][sl], want, f"guard refresh {name}")
