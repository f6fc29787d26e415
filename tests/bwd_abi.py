"""TEST INFRASTRUCTURE: the argument contract of the backward ABI as a table of violating calls (tests/test_abi_cpu.py, tests/test_bwd_sweep_gpu.py).

Every entry point has ONE legal call (small sizes, every pointer a buffer of its own) and a list of violations, each an override of that call that breaks
exactly one constraint of include/motioned.h / the launcher's checks.  A violating call must come back ME_EINVAL from the HOST with a message that names the
entry point.  Pointers come from a provider: fake, aligned addresses without a device (a call that were NOT refused would reach hipLaunchKernelGGL and come
back ME_EHIP, which the test reports), sentinel-filled device buffers on the GPU (which must stay bitwise what they were)."""
from __future__ import annotations

import ctypes as C

NULL, OFF = "null", "off"      # pointer overrides: NULL, or ("off", bytes): the buffer's address moved by that many bytes (misalignment)


def _f16(n):
    return 2 * n


def _f32(n):
    return 4 * n


# entry -> (ordered argument list [(name, kind, value)], violations [(label, {name: override}, substring the message must hold)])
#   kind "p": pointer to a buffer of `value` bytes ("po": an OUTPUT, sentinel-checked); "i" / "f": scalar; the stream is appended by the caller
def _table(L):
    T = {}
    M, N, K = 64, 64, 64
    T["me_gemm_dw"] = ("struct:GemmDwArgs", [
        ("dY", "p", _f32(M * N)), ("X", "p", _f16(M * K)), ("dW", "po", _f32(N * 3 * K)), ("work", "po", int(L.me_gemm_dw_work_bytes(M, N, K))),
        ("M", "i", M), ("N", "i", N), ("K", "i", K), ("lddy", "i", N), ("ldx", "i", K), ("dy_is_f16", "i", 0),
        ("taps", "i", 1), ("tap", "i", 0), ("gather", "i", 0), ("frames", "i", 0), ("npix", "i", 0), ("chunk", "i", 0), ("alpha", "f", 1.0)], [
        ("null dY", {"dY": NULL}, "null"), ("null X", {"X": NULL}, "null"), ("null dW", {"dW": NULL}, "null"), ("null work", {"work": NULL}, "null"),
        ("M = 0", {"M": 0}, "multiples"), ("N not a multiple of 8", {"N": 60}, "multiples"), ("K not a multiple of 8", {"K": 60}, "multiples"),
        ("ldx not a multiple of 8", {"ldx": 68}, "multiples"), ("fp32 lddy not a multiple of 4", {"lddy": 66}, "multiples"),
        ("fp16 lddy not a multiple of 8", {"lddy": 68, "dy_is_f16": 1}, "multiples"),
        ("misaligned dY", {"dY": (OFF, 4)}, "misaligned"), ("misaligned X", {"X": (OFF, 8)}, "misaligned"), ("misaligned dW", {"dW": (OFF, 4)}, "misaligned"),
        ("misaligned work", {"work": (OFF, 8)}, "misaligned"),
        ("tap beyond taps", {"tap": 1}, "tap"), ("taps = 0", {"taps": 0}, "tap"), ("negative tap", {"tap": -1}, "tap"),
        ("a 3 x 3 convolution gather", {"gather": 1, "taps": 9}, "dense and TemporalConv"),
        ("TemporalConv with one tap", {"gather": 2, "frames": 4, "npix": 16, "chunk": 4}, "tconv"),
        ("TemporalConv with zero frames", {"gather": 2, "taps": 3, "frames": 0, "npix": 16, "chunk": 4}, "tconv"),
        ("TemporalConv with zero chunk", {"gather": 2, "taps": 3, "frames": 4, "npix": 16, "chunk": 0}, "tconv"),
        ("TemporalConv rows not whole clips", {"gather": 2, "taps": 3, "frames": 5, "npix": 16, "chunk": 5}, "tconv"),
        ("a dense layer with three taps", {"taps": 3}, "one tap")])
    heads, dh, nq, nk = 8, 40, 16, 16
    Cc = heads * dh
    T["me_attn_bwd"] = ("struct:AttnBwdArgs", [
        ("Q", "p", _f16(nq * Cc)), ("K", "p", _f16(nk * Cc)), ("V", "p", _f16(nk * Cc)), ("O", "p", _f16(nq * Cc)), ("dO", "p", _f32(nq * Cc)), ("lse", "p", _f32(nq * heads)),
        ("dQ", "po", _f32(nq * Cc)), ("dK", "po", _f32(nk * Cc)), ("dV", "po", _f32(nk * Cc)), ("delta", "po", _f32(nq * heads)),
        ("ldq", "i", Cc), ("ldk", "i", Cc), ("ldv", "i", Cc), ("ldo", "i", Cc), ("lddo", "i", Cc), ("lddq", "i", Cc), ("lddk", "i", Cc), ("lddv", "i", Cc),
        ("heads", "i", heads), ("dh", "i", dh), ("n_items", "i", 1), ("nq", "i", nq), ("nk", "i", nk), ("nseg", "i", 1), ("n_kv_items", "i", 1),
        ("seg_item", "p", 16), ("inv_ptr", "p", 16), ("inv_item", "p", 16), ("scale", "f", dh ** -0.5)], [
        ("null lse", {"lse": NULL}, "null"), ("null delta", {"delta": NULL}, "null"), ("null dK", {"dK": NULL}, "null"), ("null inv_ptr", {"inv_ptr": NULL}, "null"),
        ("no items", {"n_items": 0}, "sizes"), ("no kv items", {"n_kv_items": 0}, "sizes"), ("nq = 0", {"nq": 0}, "sizes"), ("nk = 0", {"nk": 0}, "sizes"),
        ("heads = 0", {"heads": 0}, "sizes"), ("four segments", {"nseg": 4}, "sizes"), ("no segment", {"nseg": 0}, "sizes"),
        ("ldq not a multiple of 8", {"ldq": Cc + 4}, "strides"), ("ldo not a multiple of 8", {"ldo": Cc + 4}, "strides"),
        ("lddq not a multiple of 4", {"lddq": Cc + 2}, "strides"), ("lddo not a multiple of 4", {"lddo": Cc + 2}, "strides"),
        ("misaligned Q", {"Q": (OFF, 8)}, "misaligned"), ("misaligned dO", {"dO": (OFF, 4)}, "misaligned"), ("misaligned dV", {"dV": (OFF, 8)}, "misaligned"),
        ("ldq narrower than heads * dh", {"ldq": Cc - 8}, "cover"), ("ldv narrower than heads * dh", {"ldv": 8}, "cover"), ("ldo narrower than heads * dh", {"ldo": 0}, "cover"),
        ("lddo narrower than heads * dh", {"lddo": Cc - 4}, "cover"), ("lddq narrower than heads * dh", {"lddq": Cc - 4}, "cover"),
        ("lddk narrower than heads * dh", {"lddk": 0}, "cover"), ("lddv narrower than heads * dh", {"lddv": 4}, "cover"),
        ("head dim 64", {"dh": 64, "heads": 5}, "head dim")])
    B_, F_, npix = 1, 4, 2
    rows = B_ * F_ * npix
    T["me_tattn_bwd"] = ("args", [
        ("dq", "po", _f32(rows * Cc)), ("lddq", "i", Cc), ("dk", "po", _f32(rows * Cc)), ("lddk", "i", Cc), ("dv", "po", _f32(rows * Cc)), ("lddv", "i", Cc),
        ("q", "p", _f16(rows * Cc)), ("ldq", "i", Cc), ("k", "p", _f16(rows * Cc)), ("ldk", "i", Cc), ("v", "p", _f16(rows * Cc)), ("ldv", "i", Cc),
        ("dout", "p", _f32(rows * Cc)), ("lddo", "i", Cc), ("batch", "i", B_), ("frames", "i", F_), ("npix", "i", npix), ("heads", "i", heads), ("dh", "i", dh),
        ("scale", "f", dh ** -0.5)], [
        ("null dq", {"dq": NULL}, "bad arguments"), ("null v", {"v": NULL}, "bad arguments"), ("null dout", {"dout": NULL}, "bad arguments"),
        ("batch = 0", {"batch": 0}, "bad arguments"), ("frames = 0", {"frames": 0}, "bad arguments"), ("65 frames", {"frames": 65}, "frames <= 64"),
        ("npix = 0", {"npix": 0}, "bad arguments"), ("heads = 0", {"heads": 0}, "bad arguments"), ("dh = 0", {"dh": 0}, "bad arguments"),
        ("head dim 64", {"dh": 64}, "head dim"), ("head dim 48", {"dh": 48}, "head dim"),
        ("ldq narrower than the row", {"ldq": Cc - 8}, "strides"), ("ldv narrower than the row", {"ldv": 8}, "strides"),
        ("lddo narrower than the row", {"lddo": Cc - 4}, "strides"), ("lddk narrower than the row", {"lddk": 0}, "strides"),
        ("64 frames of head dim 160", {"frames": 64, "dh": 160, "heads": 2, "npix": 0 + 1, "batch": 1, "ldq": 320, "ldk": 320, "ldv": 320, "lddo": 320, "lddq": 320,
                                        "lddk": 320, "lddv": 320}, "LDS")])
    grows, rpg, Cg = 16, 8, 64
    T["me_groupnorm_bwd"] = ("args", [
        ("dx", "po", _f32(grows * Cg)), ("lddx", "i", Cg), ("x", "p", _f16(grows * Cg)), ("ldx", "i", Cg), ("gamma", "p", _f16(Cg)), ("beta", "p", _f16(Cg)),
        ("dy", "p", _f32(grows * Cg)), ("lddy", "i", Cg), ("rows", "i", grows), ("rows_per_group", "i", rpg), ("C", "i", Cg), ("groups", "i", 32), ("eps", "f", 1e-5),
        ("silu", "i", 1), ("scratch", "po", int(L.me_groupnorm_bwd_scratch_bytes(grows, rpg, 32)))], [
        ("null dx", {"dx": NULL}, "bad arguments"), ("null beta", {"beta": NULL}, "bad arguments"), ("null scratch", {"scratch": NULL}, "bad arguments"),
        ("rows = 0", {"rows": 0}, "bad arguments"), ("rows_per_group = 0", {"rows_per_group": 0}, "bad arguments"),
        ("rows not whole groups", {"rows_per_group": 5}, "bad arguments"), ("groups = 0", {"groups": 0}, "bad channels"), ("65 groups", {"groups": 65, "C": 65 * 8}, "bad channels"),
        ("C not a multiple of groups", {"C": 72, "ldx": 72, "lddx": 72, "lddy": 72}, "bad channels"),
        ("C not a multiple of 8", {"C": 36, "groups": 4, "ldx": 40, "lddx": 36, "lddy": 36}, "bad channels"),
        ("C beyond 2560", {"C": 2592, "ldx": 2592, "lddx": 2592, "lddy": 2592}, "bad channels"),
        ("ldx not a multiple of 8", {"ldx": Cg + 4}, "strides"), ("lddx not a multiple of 4", {"lddx": Cg + 2}, "strides"), ("lddy not a multiple of 4", {"lddy": Cg + 2}, "strides"),
        ("misaligned dx", {"dx": (OFF, 4)}, "misaligned"), ("misaligned x", {"x": (OFF, 8)}, "misaligned"), ("misaligned gamma", {"gamma": (OFF, 2)}, "misaligned"),
        ("misaligned dy", {"dy": (OFF, 8)}, "misaligned"), ("misaligned scratch", {"scratch": (OFF, 8)}, "misaligned")])
    lrows, Cl = 5, 320
    T["me_layernorm_bwd"] = ("args", [
        ("dx", "po", _f32(lrows * Cl)), ("lddx", "i", Cl), ("x", "p", _f16(lrows * Cl)), ("ldx", "i", Cl), ("gamma", "p", _f16(Cl)), ("dy", "p", _f32(lrows * Cl)),
        ("lddy", "i", Cl), ("rows", "i", lrows), ("C", "i", Cl), ("eps", "f", 1e-5)], [
        ("null dx", {"dx": NULL}, "bad arguments"), ("null x", {"x": NULL}, "bad arguments"), ("null gamma", {"gamma": NULL}, "bad arguments"),
        ("null dy", {"dy": NULL}, "bad arguments"), ("rows = 0", {"rows": 0}, "bad arguments"), ("C = 0", {"C": 0}, "bad arguments"),
        ("ldx narrower than C", {"ldx": Cl - 8}, "strides"), ("lddx narrower than C", {"lddx": Cl - 4}, "strides"), ("lddy narrower than C", {"lddy": 0}, "strides"),
        ("dx off its element size", {"dx": (OFF, 2)}, "misaligned"), ("dy off its element size", {"dy": (OFF, 1)}, "misaligned"), ("x off its element size", {"x": (OFF, 1)}, "misaligned"),
        ("gamma off its element size", {"gamma": (OFF, 1)}, "misaligned")])
    T["me_geglu_bwd"] = ("args", [
        ("dpre", "po", _f16(4 * 64)), ("ldd", "i", 64), ("pre", "p", _f16(4 * 64)), ("ldp", "i", 64), ("dy", "p", _f32(4 * 32)), ("lddy", "i", 32), ("M", "i", 4), ("N", "i", 64)], [
        ("null dpre", {"dpre": NULL}, "bad arguments"), ("null pre", {"pre": NULL}, "bad arguments"), ("null dy", {"dy": NULL}, "bad arguments"),
        ("M = 0", {"M": 0}, "bad arguments"), ("N = 0", {"N": 0}, "bad arguments"), ("N not a multiple of 32", {"N": 48}, "multiple of 32"),
        ("ldd narrower than N", {"ldd": 32}, "strides"), ("ldp narrower than N", {"ldp": 56}, "strides"), ("lddy narrower than N / 2", {"lddy": 0}, "strides"),
        ("dpre off its element size", {"dpre": (OFF, 1)}, "misaligned"), ("pre off its element size", {"pre": (OFF, 1)}, "misaligned"),
        ("dy off its element size", {"dy": (OFF, 2)}, "misaligned")])
    T["me_softmax_bwd_rows"] = ("args", [
        ("dS", "po", _f16(4 * 64)), ("ldds", "i", 64), ("P", "p", _f16(4 * 64)), ("ldp", "i", 64), ("dP", "p", _f16(4 * 64)), ("lddp", "i", 64), ("rows", "i", 4), ("cols", "i", 64),
        ("scale", "f", 1.0)], [
        ("null dS", {"dS": NULL}, "bad arguments"), ("null P", {"P": NULL}, "bad arguments"), ("null dP", {"dP": NULL}, "bad arguments"),
        ("rows = 0", {"rows": 0}, "bad arguments"), ("cols = 0", {"cols": 0}, "bad arguments"), ("cols not a multiple of 8", {"cols": 60}, "multiples of 8"),
        ("ldds not a multiple of 8", {"ldds": 68}, "multiples of 8"), ("ldp not a multiple of 8", {"ldp": 68}, "multiples of 8"), ("lddp not a multiple of 8", {"lddp": 68}, "multiples of 8"),
        ("misaligned dS", {"dS": (OFF, 8)}, "aligned"), ("misaligned P", {"P": (OFF, 2)}, "aligned"), ("misaligned dP", {"dP": (OFF, 4)}, "aligned")])
    T["me_colsum"] = ("args", [
        ("out", "po", _f32(64)), ("dY", "p", _f32(8 * 64)), ("lddy", "i", 64), ("dy_is_f16", "i", 0), ("M", "i", 8), ("N", "i", 64), ("alpha", "f", 1.0),
        ("work", "po", int(L.me_colsum_work_bytes(64)))], [
        ("null out", {"out": NULL}, "bad arguments"), ("null dY", {"dY": NULL}, "bad arguments"), ("null work", {"work": NULL}, "bad arguments"),
        ("M = 0", {"M": 0}, "bad arguments"), ("N = 0", {"N": 0}, "bad arguments"), ("negative M", {"M": -8}, "bad arguments"),
        ("lddy narrower than N", {"lddy": 56}, "stride"), ("fp16 lddy narrower than N", {"lddy": 0, "dy_is_f16": 1}, "stride"),
        ("fp32 dY off its element size", {"dY": (OFF, 2)}, "misaligned"), ("fp16 dY off its element size", {"dY": (OFF, 1), "dy_is_f16": 1}, "misaligned"),
        ("out off its element size", {"out": (OFF, 2)}, "misaligned"), ("work off its element size", {"work": (OFF, 1)}, "misaligned")])
    T["me_sumsq_absmax"] = ("args", [
        ("out", "po", _f32(2)), ("x", "p", _f32(100)), ("n", "i", 100), ("work", "po", int(L.me_sumsq_work_bytes()))], [
        ("null out", {"out": NULL}, "bad arguments"), ("null x", {"x": NULL}, "bad arguments"), ("null work", {"work": NULL}, "bad arguments"), ("n = 0", {"n": 0}, "bad arguments"),
        ("negative n", {"n": -1}, "bad arguments")])
    T["me_adamw"] = ("args", [
        ("p", "po", _f32(100)), ("m", "po", _f32(100)), ("v", "po", _f32(100)), ("g", "p", _f32(100)), ("n", "i", 100), ("lr", "f", 1e-3), ("beta1", "f", 0.9), ("beta2", "f", 0.999),
        ("eps", "f", 1e-8), ("weight_decay", "f", 1e-2), ("bias_c1", "f", 0.1), ("bias_c2", "f", 0.001), ("gnorm_sq", "p", _f32(2)), ("max_grad_norm", "f", 1.0),
        ("grad_scale", "f", 1.0)], [
        ("null p", {"p": NULL}, "bad arguments"), ("null m", {"m": NULL}, "bad arguments"), ("null v", {"v": NULL}, "bad arguments"), ("null g", {"g": NULL}, "bad arguments"),
        ("n = 0", {"n": 0}, "bad arguments"), ("bias_c1 = 0", {"bias_c1": 0.0}, "bad arguments"), ("negative bias_c2", {"bias_c2": -1.0}, "bad arguments")])
    return T


def entries(L):
    return _table(L)


def violation_ids(L=None):
    """(entry, label) of every violation; the labels need no library (sizes only matter for the buffers)."""
    class _Sizes:
        def __getattr__(self, n):
            return lambda *a: 64
    return [(e, lab) for e, (_, _, vs) in _table(L or _Sizes()).items() for lab, _, _ in vs]


def call(L, capi, entry, spec, overrides, ptr):
    """One call of `entry` with the legal arguments of `spec` and `overrides` applied; ptr(name, nbytes) -> address.  Returns the entry point's status."""
    kind, args, _ = spec
    vals = []
    for name, k, v in args:
        o = overrides.get(name, None)
        if k in ("p", "po"):
            a = ptr(name, v)
            if o == NULL:
                a = None
            elif isinstance(o, tuple) and o[0] == OFF:
                a = a + o[1]
            vals.append(a)
        else:
            vals.append(v if o is None else o)
    fn = getattr(L, entry)
    if kind.startswith("struct:"):
        st = getattr(capi, kind.split(":")[1])()
        for (name, _, _), v in zip(args, vals):
            setattr(st, name, v)
        return fn(C.byref(st), None)
    return fn(*vals, None)
