"""TEST INFRASTRUCTURE: one refused call per host-side constraint the forward kernels rely on (me_gemm, me_attn, me_tattn, me_groupnorm, me_layernorm,
me_softmax_rows, me_ln_stats), as tests/bwd_abi.py does for the backward family.  Every constraint was found by READING the launch code (csrc/gemm.hip
me_gemm / gemm_dispatch, csrc/attn.hip me_attn, csrc/tattn.hip me_tattn, csrc/norm.hip); no violating call is ever launched: each is refused on the host.

tables(capi) yields (entry point, make, bad): make(ptr) builds the arguments of a VALID call from ptr(name, bytes) -> address (a device buffer on the GPU,
a fabricated address without one); bad lists (label, change(arguments, ptr), a needle of the refusal message).  EVERY address of a call, the ones a change
adds included, comes from ptr: should a host check ever regress, the call lands in buffers the test owns.

Constraints this sweep added to the entry points because the kernels assumed them unchecked: me_tattn's per-thread kernel is built for 512 threads per
block, (320 / dh) * query frames (`threads`); me_attn's general-dual kernel reads mask plane `head` of the 8 the ABI gives it and dereferences mask
(`mask planes`); me_groupnorm's scratch holds float4 partial sums behind the fp64 statistics (`stats alignment`)."""
import ctypes as C
from types import SimpleNamespace


def _set(**kw):
    """Field = value; a callable value is given ptr and returns the address to set."""
    def change(a, ptr):
        for k, v in kw.items():
            setattr(a, k, v(ptr) if callable(v) else v)
    return change


def _bump(name, by):
    def change(a, ptr):
        setattr(a, name, (getattr(a, name) or 0) + by)
    return change


def _at(name, nbytes, off=0):
    return lambda ptr: ptr(name, nbytes) + off


def tables(capi):
    def gemm(ptr):
        a = capi.GemmArgs()
        a.M, a.N, a.K, a.ldx, a.ldc, a.alpha = 64, 64, 64, 64, 64, 1.0
        a.X, a.W, a.C = ptr("x", 64 * 64 * 2), ptr("w", 64 * 64 * 2), ptr("c", 64 * 64 * 2)
        a.bias, a.rowvec, a.res = ptr("bias", 128), ptr("rowvec", 64 * 64 * 2), ptr("res", 64 * 64 * 2)
        a.ldrv, a.rows_per_vec, a.ldr = 64, 8, 64
        return a

    def gemm_c2(ptr):
        a = gemm(ptr)
        a.rowvec = a.res = None
        a.C2, a.c2_col0, a.c2_dh, a.c2_hs = ptr("c2", 64 * 64 * 2), 32, 16, 64 * 16
        return a

    def gemm_ln(ptr):
        a = gemm(ptr)
        a.bias = a.rowvec = a.res = None
        a.ln_stats, a.ln_colsum, a.ln_cvec = ptr("st", 64 * 2 * 4), ptr("cs", 64 * 4), ptr("cv", 64 * 4)
        a.ln_stride, a.ln_parts, a.ln_eps = 128, 1, 1e-5
        a.ln_out, a.ln_out_stride = ptr("so", 64 * 2 * 4), 128
        return a

    def gemm_conv(ptr):
        a = gemm(ptr)
        a.gather, a.Hin, a.Win, a.Hout, a.Wout, a.stride = capi.GATHER_CONV3, 8, 8, 8, 8, 1
        a.W = ptr("w9", 64 * 9 * 64 * 2)
        return a

    yield "me_gemm", gemm, [
        ("K % 8", _set(K=60), "multiples of 8"), ("ldx % 8", _set(ldx=68), "multiples of 8"), ("N % 4", _set(N=62), "multiples of 8"), ("ldc % 4", _set(ldc=66), "multiples of 8"),
        ("X off 16 bytes", _bump("X", 8), "misaligned pointer"), ("W off 16 bytes", _bump("W", 8), "misaligned pointer"), ("C off 8 bytes", _bump("C", 4), "misaligned pointer"),
        ("bias off 8 bytes", _bump("bias", 4), "misaligned bias"), ("rows_per_vec 0", _set(rows_per_vec=0), "bad rowvec"), ("ldrv % 4", _set(ldrv=66), "bad rowvec"),
        ("rowvec off 8 bytes", _bump("rowvec", 4), "bad rowvec"), ("ldr % 4", _set(ldr=66), "bad residual"), ("res off 8 bytes", _bump("res", 4), "bad residual"),
        ("act 3", _set(act=3), "bad activation"), ("res_rows < 0", _set(res_rows=-1), "negative res_rows"), ("geglu with terms", _set(geglu=1), "geglu needs"),
        ("m_off >= M", _set(m_off=64), "m_off"), ("gather 3", _set(gather=3), "bad gather mode"), ("M 0", _set(M=0), "non-positive"),
    ]
    yield "me_gemm", gemm_c2, [
        ("c2_dh % 8", _set(c2_dh=4), "head-major"), ("c2_col0 % 16", _set(c2_col0=8), "head-major"), ("partial head", _set(c2_dh=24), "head-major"),
        ("c2_hs < M c2_dh", _set(c2_hs=63 * 16), "head-major"), ("C2 off 16 bytes", _bump("C2", 8), "head-major"), ("C2 with act", _set(act=1), "head-major"),
    ]
    yield "me_gemm", gemm_ln, [
        ("ln with bias", _set(bias=_at("bias", 128)), "LayerNorm-folded"), ("ln with alpha", _set(alpha=0.5), "LayerNorm-folded"), ("ln_parts 5", _set(ln_parts=5), "LayerNorm-folded"),
        ("ln_stride < 2 M", _set(ln_stride=126), "LayerNorm-folded"), ("ln_colsum off 16 bytes", _bump("ln_colsum", 8), "LayerNorm-folded"), ("ln_eps 0", _set(ln_eps=0.0), "LayerNorm-folded"),
        ("ln_out with ldc % 8", _set(ldc=68), "ln_out needs"), ("ln_out stride odd", _set(ln_out_stride=129), "ln_out needs"), ("ln_out off 8 bytes", _bump("ln_out", 4), "ln_out needs"),
    ]
    yield "me_gemm", gemm_conv, [
        ("M % (Hout Wout)", _set(M=60, rowvec=None, res=None), "bad conv geometry"), ("stride 3", _set(stride=3), "bad conv geometry"), ("pad0 2", _set(pad0=2), "bad conv geometry"),
        ("ups 3 with Hout != 2 Hin", _set(ups=3), "ups = 3"), ("m_off with a convolution", _set(m_off=1), "m_off"),
    ]

    def attn(ptr):
        a = capi.AttnArgs()
        a.heads, a.dh, a.n_items, a.nq, a.nk, a.nseg, a.scale = 2, 40, 1, 16, 16, 1, 0.158
        a.ldq = a.ldk = a.ldv = a.ldo = 80
        for n in ("Q", "K", "V", "O"):
            setattr(a, n, ptr(n, 16 * 80 * 2))
        a.seg_item, a.seg_mode = ptr("si", 16), ptr("sm", 16)
        return a

    mask, lse, vsum = _at("mask", 8 * 16 * 2), _at("lse", 16 * 2 * 4), _at("vsum", 17 * 80 * 4)
    yield "me_attn", attn, [
        ("nseg 4", _set(nseg=4), "bad sizes"), ("ldq % 8", _set(ldq=84), "row strides"), ("ldo % 4", _set(ldo=82), "row strides"), ("Q off 16 bytes", _bump("Q", 8), "misaligned pointer"),
        ("O off 8 bytes", _bump("O", 4), "misaligned pointer"), ("q_items with general dual", _set(general_dual=1, mask=mask, q_items=1), "general-dual"),
        ("lse with general dual", _set(general_dual=1, mask=mask, lse=lse), "general-dual"), ("lse with vsum", _set(lse=lse, vsum=vsum), "plain segments"),
        ("hsk % 8", _set(hsk=20), "head strides"), ("item_order off 4 bytes", _set(item_order=_at("order", 16, 2)), "item_order"), ("vsum without n_kv_items", _set(vsum=vsum), "n_kv_items"),
        ("vsum off 16 bytes", _set(vsum=_at("vsum", 17 * 80 * 4, 8), n_kv_items=1), "vsum needs"), ("dh 64", _set(dh=64), "head dim"),
        ("mask planes: general dual without a mask", _set(general_dual=1), "mask"), ("mask planes: general dual with 9 heads", _set(general_dual=1, mask=mask, heads=9), "mask"),
    ]

    def tattn(ptr):
        a = capi.TAttnArgs()
        a.heads, a.dh, a.batch, a.frames, a.npix, a.scale = 8, 40, 2, 8, 1, 0.158
        a.ldq = a.ldk = a.ldv = a.ldo = 320
        for n in ("Q", "K", "V", "O"):
            setattr(a, n, ptr(n, 16 * 320 * 2))
        a.kv_map[1] = 1
        return a

    def kv_map_out_of_range(a, ptr):
        a.kv_map[1] = 2

    yield "me_tattn", tattn, [
        ("batch 9", _set(batch=9), "bad sizes"), ("dh 48", _set(dh=48, heads=20), "head dim"), ("heads dh % 320", _set(heads=7), "head dim"), ("ldo % 8", _set(ldo=324), "row strides"),
        ("O off 16 bytes", _bump("O", 8), "misaligned pointer"), ("q_frame0 + q_frames > frames", _set(q_frames=4, q_frame0=5), "frame-shard"), ("frames % kv_parts", _set(kv_parts=3), "frame-shard"),
        ("q_parts != kv_parts", _set(q_parts=2, kv_parts=4), "frame-shard"), ("kv_map out of range", kv_map_out_of_range, "kv_map"),
        ("per-thread form at 12 frames", _set(dh=32, heads=10, frames=12), "frames must be one of"), ("threads: 40 heads x 16 frames", _set(dh=8, heads=40, frames=16), "512 threads"),
    ]

    def gn(ptr):
        a = capi.GroupNormArgs()
        a.rows, a.rows_per_group, a.C, a.ldx, a.ldy, a.groups, a.eps = 16, 8, 64, 64, 64, 32, 1e-5
        a.X, a.Y, a.gamma, a.beta, a.stats = ptr("x", 2048), ptr("y", 2048), ptr("g", 128), ptr("b", 128), ptr("stats", 4096)
        return a

    gn_bad = [("rows % rows_per_group", _set(rows_per_group=7), "multiple of rows_per_group"), ("C % groups", _set(C=72, ldx=72, ldy=72), "channel geometry"),
              ("ldy % 8", _set(ldy=68), "channel geometry"), ("gamma off 16 bytes", _bump("gamma", 8), "misaligned pointer"), ("stats alignment", _bump("stats", 8), "misaligned pointer")]
    yield "me_groupnorm", gn, gn_bad + [("C 2568", _set(C=2592, ldx=2592, ldy=2592), "C must be <= 2560")]
    yield "me_groupnorm_apply", gn, gn_bad[:1] + gn_bad[-1:]

    def ln(ptr):
        a = capi.LayerNormArgs()
        a.rows, a.C, a.ldx, a.ldy, a.eps = 4, 64, 64, 64, 1e-5
        a.X, a.Y, a.gamma, a.beta = ptr("x", 512), ptr("y", 512), ptr("g", 128), ptr("b", 128)
        return a

    yield "me_layernorm", ln, [("C % 8", _set(C=60), "multiple of 8"), ("C 1544", _set(C=1544, ldx=1544, ldy=1544), "multiple of 8"), ("ldx % 8", _set(ldx=68), "multiple of 8"),
                               ("Y off 16 bytes", _bump("Y", 8), "misaligned pointer")]

    def softmax(ptr):
        return SimpleNamespace(Y=ptr("y", 4 * 72 * 2), ldy=72, X=ptr("x", 4 * 72 * 2), ldx=72, rows=4, cols=64)

    yield "me_softmax_rows", softmax, [("cols % 8", _set(cols=60), "multiple of 8"), ("cols 8200", _set(cols=8200, ldx=8200, ldy=8200), "multiple of 8"), ("ldx % 8", _set(ldx=68), "multiple of 8"),
                                       ("ldy % 8", _set(ldy=68), "multiple of 8"), ("X off 16 bytes", _bump("X", 8), "misaligned pointer"), ("Y off 16 bytes", _bump("Y", 8), "misaligned pointer"),
                                       ("rows 0", _set(rows=0), "multiple of 8")]

    def ln_stats(ptr):
        return SimpleNamespace(X=ptr("x", 4 * 640 * 2), ldx=640, rows=4, C=640, stats=ptr("stats", 2 * 8 * 4), stride=8)

    yield "me_ln_stats", ln_stats, [("C % 8", _set(C=636), "multiple of 8"), ("C 1544", _set(C=1544, ldx=1544), "multiple of 8"), ("ldx % 8", _set(ldx=644), "multiple of 8"),
                                    ("X off 16 bytes", _bump("X", 8), "multiple of 8"), ("stats off 8 bytes", _bump("stats", 4), "multiple of 8"), ("stride odd", _set(stride=9), "multiple of 8"),
                                    ("parts closer than 2 rows", _set(stride=6), "multiple of 8")]


def call(L, entry, a):
    if entry == "me_softmax_rows":
        return L.me_softmax_rows(a.Y, a.ldy, a.X, a.ldx, a.rows, a.cols, None)
    if entry == "me_ln_stats":
        return L.me_ln_stats(a.X, a.ldx, a.rows, a.C, a.stats, a.stride, None)
    if entry == "me_groupnorm_apply":
        return L.me_groupnorm_apply(C.byref(a), a.rows_per_group, None)
    return getattr(L, entry)(C.byref(a), None)
