"""TEST INFRASTRUCTURE: the case table of the forward sweep (tests/test_fwd_sweep_cpu.py, tests/test_fwd_sweep_gpu.py) and a Python restatement of the
forward dispatch: gemm_target / gemm_epilogue (csrc/gemm.hip gemm_dispatch, choose_split, launch_gemm, launch_gemm8p), attn_target (csrc/attn.hip me_attn)
and tattn_target (csrc/tattn.hip me_tattn).  Each returns the string me_last_kernel holds after the launch; the GPU file checks it per case.

Pure data and seeded input builders on the machinery of tests/bwd_cases.py (Case, seed_of, the bound rules); nothing here imports the HIP side.  A case
names its entry point (the ``motioneditor_amd.ops`` function), the parameters its builder turns into tensors, the per-call switches it sets around its one
launch (`env`) and the kernel the restatement predicts (`path`).  Large-grid kernels are reached at small shapes ONLY through switches the library reads
per call (ME_GEMM_BIG_MIN, ME_GEMM_8P, ME_GEMM_8P_192, ME_GEMM_8P_128, ME_GEMM_192_MINK, ME_GEMM_GEGLU_MIN, ME_GEMM_N64_BELOW, ME_GEMM_SPLITK,
ME_GEMM_ROWEPI, ME_ATTN_KVRES, ME_ATTN_80_QT2).  Switches read once per process are never set (ME_CONV_HALO_MIN, ME_CONV_HALO, ME_GEMM_BUF, ME_GEMM_STAGE,
ME_GEMM_TILE160, ME_GEMM_TILE_ORDER, ME_ATTN_FOLD, ME_TATTN_MFMA), so:
  * the halo kernel has ONE case at its smallest real grid (512 images of 16 x 16, N = 320, K = 64), marked prod;
  * the register-staged kernels (ME_GEMM_STAGE=reg) and the per-thread temporal kernel at dh 40 / 80 / 160 below 65 frames are OUT OF SCOPE.

What the restatement found unreachable (and the table therefore does not hold): the `S > nit / 4` clamp of choose_split cannot bind behind `nit >= 32`
(S <= 4 <= 8); `C2 with epilogue terms` is refused by me_gemm before launch_gemm8p could leave the row pass for it; the per-thread temporal kernel at
dh = 8 takes (320 / 8) * frames threads per block, more than the 512 it is built for from 16 frames on (me_tattn refuses those; dh = 8 runs at 8 frames).
The kernel names do not carry the staging (buffer / global_load_lds), the epilogue or the ups = 3 instantiation: those are reached by construction (K % 64,
the term set, ups) and restated by gemm_epilogue / gemm_staging, witnessed only through the result.

Bounds are the project's own per entry point (tests/test_kernels_gpu.py), restated by name in BOUNDS; `bound=`, `elementwise=` and `zero=` are the rules of
tests/bwd_cases.py.  No case uses `bound=`."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from bwd_cases import MAX_REL, REL_L2, Case, seed_of   # noqa: F401  (seed_of: re-exported for the runners)

BOUNDS: Dict[str, Tuple[float, float]] = {
    "gemm": (REL_L2, MAX_REL),                   # check() defaults of tests/test_kernels_gpu.py: fp16 storage, fp32 accumulation
    "gemm.ln_out": (1e-5, 1e-3),                 # test_gemm_ln_out_...: "row sums" against the sums of the fp16 output the launch stored
    "attention": (REL_L2, MAX_REL),
    "attention.lse": (2e-2, 0.0),                # ABSOLUTE, in log2 units: bwd_run._cmp_bounded "log-sum-exp stashed by the forward"
    "temporal_attention": (REL_L2, MAX_REL),
    "groupnorm": (REL_L2, MAX_REL),
    "layernorm": (REL_L2, MAX_REL),
    "softmax_rows": (REL_L2, MAX_REL),           # test_softmax_rows: max / mean <= MAX_REL * cols (peaked rows), applied in fwd_run.bound_of
}

# ---------------------------------------------------------------------------------------------------------------- the dispatch, restated
ENV_DEFAULTS = {"ME_GEMM_BIG_MIN": 512, "ME_GEMM_8P": 2, "ME_GEMM_8P_192": 192, "ME_GEMM_8P_128": 192, "ME_GEMM_192_MINK": 4, "ME_GEMM_GEGLU_MIN": 240,
                "ME_GEMM_N64_BELOW": 200, "ME_GEMM_SPLITK": 400, "ME_GEMM_ROWEPI": 1, "ME_ATTN_KVRES": 1, "ME_ATTN_80_QT2": 1}
HALO_MIN = 512                                   # csrc/gemm.hip:1633 halo_min_blocks (read once: its default)
THRESHOLDS = tuple(ENV_DEFAULTS)


def _envd(env):
    e = dict(ENV_DEFAULTS)
    e.update({k: int(v) for k, v in (env or {}).items()})
    return e


def _cdiv(a, b):
    return (a + b - 1) // b


def _taps(a):
    return 9 if a.get("conv") else (3 if a.get("tconv") else 1)


def choose_split(a, blocks: int, nit: int, env=None) -> int:
    """csrc/gemm.hip:1605 choose_split.  a: dict(N, K, geglu, C2, m_off, ln, conv=(..., ups), ...)."""
    e = _envd(env)
    ups3 = bool(a.get("conv")) and a["conv"][5] == 3
    if a.get("geglu") or a["K"] % 64 or a["N"] < 1280 or blocks >= e["ME_GEMM_SPLITK"] or nit < 32 or a.get("C2") or a.get("m_off") or a.get("ln") or ups3:
        return 1
    S = min(_cdiv(640, blocks), 4)
    S = min(S, nit // 4)
    return 1 if S < 2 else S


def gemm_work_bytes(a, env=None) -> int:
    """csrc/gemm.hip:1865 me_gemm_work_bytes: the bound over the 128-row kernels' tiles."""
    if min(a["M"], a["N"], a["K"]) <= 0 or a.get("geglu") or a["K"] % 64 or a["N"] % 4:
        return 0
    S = choose_split(a, _cdiv(a["M"], 128) * _cdiv(a["N"], 160), (a["K"] // 64) * _taps(a), env)
    return 16 * a["M"] * a["N"] if S > 1 else 0


def _gemm_kernel(a, BM, BN, buf, Msel, e, env):
    """csrc/gemm.hip:1724 launch_gemm: the name, with "+splitk" when the buffer-staged launch is given scratch and choose_split splits it."""
    S = 1
    if buf and a.get("work_given", True):        # :1744: buffer-staged and given scratch
        S = choose_split(a, _cdiv(Msel, BM) * _cdiv(a["N"], BN), (a["K"] // 64) * _taps(a), env)
        if a.get("work") in ("short", "misaligned"):
            S = 1                                # :1750: too few bytes, or a pointer off 16 bytes: the unsplit launch
    return f"gemm_kernel<{BM},{BN}>" + ("+splitk" if S > 1 else "")


def gemm_target(a, env=None) -> str:
    """csrc/gemm.hip:1903 gemm_dispatch (default ME_GEMM_STAGE) -> the me_last_kernel string.  a: dict(M, N, K, conv=(Hin, Win, Hout, Wout, stride, ups[, pad0])
    | tconv=(...) | neither, geglu, sel_rows, m_off, C2, ln, work, work_given)."""
    e = _envd(env)
    conv = a.get("conv")
    pm = 4 if conv and conv[5] == 3 else 1       # :1939 ups = 3: rows per output parity
    M, N, K = a["M"] // pm, a["N"], a["K"]
    Msel = max(a.get("sel_rows", 0) // pm, M)    # :1959
    geglu, dense = bool(a.get("geglu")), not conv and not a.get("tconv")
    wide = N % 128 == 0 or N % 64 != 0           # :1951
    big_blocks = _cdiv(Msel, 256) * pm * (N // 320)
    if conv and conv[4] == 1 and conv[5] == 0 and not (len(conv) > 6 and conv[6]) and N % 320 == 0 and K % 64 == 0 and conv[0] % 16 == 0 and conv[1] % 16 == 0 \
            and not geglu and big_blocks >= HALO_MIN:
        return "conv3_halo_kernel"               # :1961
    buf = K % 64 == 0                            # :1964 (ME_GEMM_BUF default)
    nit8 = (K // 64) * ((4 if pm == 4 else 9) if conv else (3 if a.get("tconv") else 1))
    u8 = e["ME_GEMM_8P"]
    on8 = buf and u8 > 0 and nit8 >= u8
    g = "false" if dense else "true"
    lim = lambda v: v if v > 0 else 1 << 60      # noqa: E731   (:1679 / :1685: 0 = never)
    if geglu and dense and on8 and N % 256 == 0 and _cdiv(Msel, 256) * (N // 256) >= e["ME_GEMM_GEGLU_MIN"]:
        return "gemm8p_kernel<256,256,false>"    # :1968
    if N % 320 == 0 and big_blocks >= e["ME_GEMM_BIG_MIN"]:       # :1970
        if on8:
            if not geglu:
                return f"gemm8p_kernel<256,320,{g}>"
            if dense and N % 256 == 0 and _cdiv(Msel, 256) * (N // 256) >= e["ME_GEMM_BIG_MIN"]:
                return "gemm8p_kernel<256,256,false>"
        return _gemm_kernel(a, 256, 320, buf, Msel, e, env)
    k192 = nit8 >= e["ME_GEMM_192_MINK"]
    if N % 320 == 0 and not geglu and on8 and k192 and _cdiv(Msel, 192) * pm * (N // 320) >= lim(e["ME_GEMM_8P_192"]):
        return f"gemm8p_kernel<192,320,{g}>"     # :1982
    if dense and N % 320 == 0 and not geglu and on8 and k192 and _cdiv(Msel, 128) * (N // 320) >= lim(e["ME_GEMM_8P_128"]):
        return "gemm8p_kernel<128,320,false>"    # :1986
    blocks160 = _cdiv(Msel, 128) * pm * _cdiv(N, 160)
    blocks128 = _cdiv(Msel, 128) * pm * _cdiv(N, 128)
    if N % 64 == 0 and blocks128 < e["ME_GEMM_N64_BELOW"]:
        return _gemm_kernel(a, 128, 64, buf, Msel, e, env)        # :1993
    if N % 128 == 0 and blocks160 < 512:
        return _gemm_kernel(a, 128, 128, buf, Msel, e, env)       # :1995
    if not geglu and N % 160 == 0:
        return _gemm_kernel(a, 128, 160, buf, Msel, e, env)       # :1996 (ME_GEMM_TILE160 default)
    if wide:
        return _gemm_kernel(a, 128, 128, buf, Msel, e, env)       # :1997
    return _gemm_kernel(a, 128, 64, False, Msel, e, env)          # :1998: always global_load_lds-staged, never split


def gemm_staging(a) -> str:
    """buffer- or global_load_lds-staged, and the packed-tap mode of a convolution with K < 64 (8, 16, 32: whole taps per 64-wide slab; 24 is not)."""
    if a["K"] % 64 == 0:
        return "buf"
    return "glds+packed" if a.get("conv") and a["K"] in (8, 16, 32) else "glds"


def gemm_epilogue(a, env=None) -> str:
    """csrc/gemm.hip:1793 launch_gemm8p: "row<f>" (the specialised row pass of term set f) or "direct".  a also holds rowvec / res / res2 / act and the
    alignment facts c_al / rv_al / res_al / res2_al (16-byte pointer and ld % 8 == 0)."""
    e = _envd(env)
    k = gemm_target(a, env)
    if not k.startswith("gemm8p"):
        return "direct"
    f = (2 if a.get("rowvec") else 0) | (4 if a.get("res") else 0) | (8 if a.get("res2") else 0)
    al = all(a.get(n, True) for n in ("c_al", "rv_al", "res_al", "res2_al"))
    conv = a.get("conv")
    ups3 = bool(conv) and conv[5] == 3
    if "320" in k and not (ups3 and f) and e["ME_GEMM_ROWEPI"] and not a.get("geglu") and not a.get("act") and a["N"] % 320 == 0 and f in (0, 2, 4, 6, 12) and al \
            and (not a.get("C2") or f == 0):
        return f"row{f}"
    if "256,256" in k and e["ME_GEMM_ROWEPI"] and a.get("geglu") and a["N"] % 256 == 0 and a.get("c_al", True) and not a.get("C2"):
        return "row0"
    return "direct"


def gemm_ln_out_fused(a, env=None) -> bool:
    """csrc/gemm.hip:1808 g_ln_fused: the launch writes ln_out from its own epilogue (else me_gemm appends me_ln_stats)."""
    conv = a.get("conv")
    return gemm_target(a, env).startswith("gemm8p_kernel<") and ",320," in gemm_target(a, env) and gemm_epilogue(a, env).startswith("row") \
        and not (conv and conv[5] == 3)


def attn_target(a, env=None) -> str:
    """csrc/attn.hip:1443 me_attn.  a: dict(dh, nq, nk, nseg, general_dual, vsum, o_al (ldo % 8 == 0 and O 16-byte aligned))."""
    e = _envd(env)
    dh, nq, nk = a["dh"], a["nq"], a["nk"]
    if a.get("general_dual"):
        return f"attn_kernel<{dh},{1 if dh == 160 else 2},general-dual>"      # :1455
    fold = nk >= 256                             # :1475 (ME_ATTN_FOLD default)
    kvres = a.get("nseg", 1) == 1 and 64 < nk <= 80 and not a.get("vsum") and a.get("o_al", True) and e["ME_ATTN_KVRES"] != 0      # :1479
    kind = "fold" if fold else "classic"
    if dh == 40:
        if fold and nq >= 512:
            return "attn2_kernel<40,2,16,fold>"
        if kvres and nq >= 512:
            return "attn2_kernel<40,2,8,kvres>"
        return f"attn2_kernel<40,2,{8 if nq >= 256 else 4},{kind}>"
    if dh == 80:
        if kvres and nq >= 256:
            return "attn2_kernel<80,1,8,kvres>"
        if fold and nq >= 256 and e["ME_ATTN_80_QT2"] != 0:
            return "attn2_kernel<80,2,8,fold>"
        return f"attn2_kernel<80,1,8,{kind}>" if nq >= 128 else f"attn2_kernel<80,2,4,{kind}>"
    if kvres and nq >= 256:
        return "attn2_kernel<160,1,8,kvres>"
    return "attn2_kernel<160,1,4,classic>"


def attn_geometry(kernel: str) -> Tuple[int, int]:
    """(queries per block, keys per stage) of a me_attn kernel: csrc/attn.hip launch_attn2 BQ = 16 QT NW, stages of 64 NSUB keys; launch_attn BQ = 64 QT."""
    if kernel.startswith("attn_kernel"):
        return (64 if "<160" in kernel else 128), 64
    dh, qt, nw = (int(v) for v in kernel[kernel.index("<") + 1:].split(",")[:3])
    nsub = {(40, 16): 4, (40, 8): 2, (80, 8): 2 if qt == 2 or "kvres" in kernel else 1, (160, 8): 2}.get((dh, nw), 1)
    return 16 * qt * nw, 64 * nsub


def tattn_target(a) -> Optional[str]:
    """csrc/tattn.hip me_tattn (ME_TATTN_MFMA default); None: refused."""
    dh, F = a["dh"], a["frames"]
    if F <= 64 and dh in (40, 80, 160):
        return f"tattn_mfma_kernel<{dh},{64 if F > 32 else 32}>"
    if F not in (8, 16, 24, 32, 40, 48) or 320 % dh or (320 // dh) * (a.get("q_frames") or F) > 512:
        return None
    return f"tattn_kernel<{F}>"


GEMM_TARGETS = ["conv3_halo_kernel", "gemm8p_kernel<256,320,false>", "gemm8p_kernel<256,320,true>", "gemm8p_kernel<192,320,false>", "gemm8p_kernel<192,320,true>",
                "gemm8p_kernel<128,320,false>", "gemm8p_kernel<256,256,false>", "gemm_kernel<256,320>", "gemm_kernel<128,160>", "gemm_kernel<128,128>",
                "gemm_kernel<128,64>", "gemm_kernel<256,320>+splitk", "gemm_kernel<128,160>+splitk", "gemm_kernel<128,128>+splitk", "gemm_kernel<128,64>+splitk"]
ATTN_TARGETS = ["attn2_kernel<40,2,16,fold>", "attn2_kernel<40,2,8,kvres>", "attn2_kernel<40,2,8,fold>", "attn2_kernel<40,2,4,fold>", "attn2_kernel<40,2,8,classic>",
                "attn2_kernel<40,2,4,classic>", "attn2_kernel<80,1,8,kvres>", "attn2_kernel<80,2,8,fold>", "attn2_kernel<80,1,8,fold>", "attn2_kernel<80,2,4,fold>",
                "attn2_kernel<80,1,8,classic>", "attn2_kernel<80,2,4,classic>", "attn2_kernel<160,1,8,kvres>", "attn2_kernel<160,1,4,classic>",
                "attn_kernel<40,2,general-dual>", "attn_kernel<80,2,general-dual>", "attn_kernel<160,1,general-dual>"]
TATTN_TARGETS = [f"tattn_mfma_kernel<{dh},{kp}>" for dh in (40, 80, 160) for kp in (32, 64)] + [f"tattn_kernel<{F}>" for F in (8, 16, 24, 32, 40, 48)]

# ---------------------------------------------------------------------------------------------------------------- the table
CASES = []
PAIRS = []          # (threshold or parameter name, case id below / off, case id at / on): two cases that differ only in crossing it and land on different kernels


def _gemm_args(p):
    """The restatement's view of a gemm case (the full launch)."""
    a = dict(p)
    a["ln"] = bool(p.get("ln"))
    a["C2"] = p.get("head_major") is not None
    a["c_al"] = not p.get("c_off") and not p.get("c_pad")
    a["res_al"] = not p.get("res_off")
    a["work_given"] = p["N"] >= 1280 and p["M"] <= 8192 and gemm_work_bytes(a, p.get("env")) > 0      # ops.gemm asks for scratch only then
    return a


def _g(id_, prod=False, twice=False, bound=None, **p):
    a = _gemm_args(p)
    if p.get("pieces_only"):                     # the case IS its row-range launches: one kernel per piece, and a piece with m_off > 0 is never split
        cuts = [0] + list(p["pieces"]) + [p["M"]]
        p["paths"] = [gemm_target(dict(a, M=hi, m_off=lo, sel_rows=p["M"]), p.get("env")) for lo, hi in zip(cuts[:-1], cuts[1:])]
        a["m_off"] = cuts[-2]
    CASES.append(Case(id=f"gemm-{id_}", entry="gemm", p=p, path=gemm_target(a, p.get("env")), prod=prod, twice=twice, bound=bound))


def _conv(n_img, H, W, stride=1, ups=0, pad0=0):
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = ((Hv - 1) // stride + 1, (Wv - 1) // stride + 1) if not pad0 else ((Hv - 2) // stride + 1, (Wv - 2) // stride + 1)
    return dict(M=n_img * Ho * Wo, conv=(H, W, Ho, Wo, stride, ups, pad0))


# M as n_img x H x W of a 3 x 3 convolution, and as frames x npix of a TemporalConv (one batch entry, one chunk)
_AS_IMG = {1: (1, 1, 1), 127: (1, 1, 127), 128: (2, 8, 8), 129: (1, 3, 43), 191: (1, 1, 191), 192: (3, 8, 8), 193: (1, 193, 1), 255: (1, 15, 17), 256: (1, 16, 16),
           257: (1, 1, 257), 385: (1, 5, 77), 513: (1, 19, 27)}
_AS_FRAMES = {1: (1, 1), 255: (3, 85), 256: (4, 64), 257: (257, 1), 513: (19, 27), 191: (191, 1), 192: (3, 64), 193: (193, 1), 385: (5, 77)}
_E256, _E192, _E128 = {"ME_GEMM_BIG_MIN": 0}, {"ME_GEMM_8P_192": 1}, {"ME_GEMM_8P_128": 1}

# ---- the 8-phase kernels (csrc/gemm.hip gemm8p_kernel: BM x BN tiles, K tiles of 64): M in {1, BM - 1, BM, BM + 1, 2 BM + 1} ----
for _M in (1, 255, 256, 257, 513):
    _g(f"8p256-dense-M{_M}", M=_M, N=320, K=128, bias=True, env=_E256, pieces=(_M - 1,) if _M == 257 else None, sel=2 if _M == 256 else 0, twice=_M == 513)
    _g(f"8p256-conv-M{_M}", N=320, K=64, env=_E256, **_conv(*_AS_IMG[_M]))
    _g(f"8p256-tconv-M{_M}", M=_M, N=320, K=64, env=_E256, tconv=_AS_FRAMES[_M] + (_AS_FRAMES[_M][0],))
    _g(f"8p256-geglu-M{_M}", M=_M, N=256, K=128, bias=True, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0})
    _g(f"g256-dense-M{_M}", M=_M, N=320, K=64, bias=True, env=_E256, pieces=(_M - 1,) if _M == 257 else None)        # exactly ONE K tile against use_8p() = 2
for _M in (1, 191, 192, 193, 385):
    _g(f"8p192-dense-M{_M}", M=_M, N=320, K=256, bias=True, env=_E192, pieces=(_M - 1,) if _M == 193 else None, sel=2 if _M == 192 else 0, twice=_M == 385)
    _g(f"8p192-conv-M{_M}", N=320, K=64, env=_E192, **_conv(*_AS_IMG[_M]))
for _M in (1, 127, 128, 129, 257):
    _g(f"8p128-dense-M{_M}", M=_M, N=320, K=256, bias=True, env=_E128, pieces=(_M - 1,) if _M == 129 else None, sel=2 if _M == 128 else 0, twice=_M == 257)
    _g(f"g128x64-dense-M{_M}", M=_M, N=64, K=128, bias=True, pieces=(_M - 1,) if _M == 129 else None, sel=2 if _M == 128 else 0, twice=_M == 257)
    _g(f"g128x128-dense-M{_M}", M=_M, N=128, K=128, bias=True, env={"ME_GEMM_N64_BELOW": 0}, pieces=(_M - 1,) if _M == 129 else None, sel=2 if _M == 128 else 0, twice=_M == 257)
    _g(f"g128x160-dense-M{_M}", M=_M, N=160, K=128, bias=True, pieces=(_M - 1,) if _M == 129 else None, sel=2 if _M == 128 else 0, twice=_M == 257)
    _g(f"g128x64-conv-M{_M}", N=64, K=64, **_conv(*_AS_IMG[_M]))
_g("8p256-tconv-pieces", M=2 * 6 * 50, N=320, K=64, env=_E256, tconv=(6, 50, 3), pieces=(100, 599))
_g("8p256-conv-sel", N=320, K=64, env=_E256, sel=2, twice=True, **_conv(4, 9, 11))
_g("8p192-tconv-pieces", M=2 * 6 * 50, N=320, K=128, env=_E192, tconv=(6, 50, 6), pieces=(250,))
_g("g128x64-tconv-pieces", M=3 * 8 * 11, N=64, K=72, tconv=(8, 11, 4), pieces=(88, 263), twice=True)
# the second way onto the 256-wide GEGLU kernel (N % 320 == 0 and N % 256 == 0 behind ME_GEMM_BIG_MIN), and GEGLU that stays off it
_g("8p256-geglu-via-big-min", M=260, N=1280, K=128, bias=True, geglu=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_GEGLU_MIN": 1 << 30})
_g("g256-geglu-N320", M=260, N=320, K=128, bias=True, geglu=True, env=_E256)
_g("g128x128-geglu-default", M=130, N=256, K=128, bias=True, geglu=True, env={"ME_GEMM_N64_BELOW": 0})
_g("g128x64-geglu-default", M=130, N=256, K=128, bias=True, geglu=True)
_g("8p256-geglu-forced", M=130, N=256, K=128, bias=True, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0})
_g("geglu-N288-forced", M=130, N=288, K=128, bias=True, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0})
_g("8p256-geglu-N512-no-bias", M=300, N=512, K=192, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0}, twice=True, sel=2)

# ---- N on each side of every divisibility test of gemm_dispatch (% 320, % 256, % 160, % 128, % 64), N tails of the 128-row kernels, the smallest N ----
for _N in (4, 36, 68, 132, 164, 196):
    _g(f"g128x128-N{_N}-tail", M=130, N=_N, K=128, bias=True, rowvec=50)
for _N, _env in ((64, None), (68, None), (164, None), (64, {"ME_GEMM_N64_BELOW": 0}), (192, {"ME_GEMM_N64_BELOW": 0}), (128, None), (128, {"ME_GEMM_N64_BELOW": 0}), (160, None), (320, None),
                 (320, {"ME_GEMM_N64_BELOW": 0}), (480, None), (640, {"ME_GEMM_N64_BELOW": 0}), (256, _E256), (316, _E256), (320, _E256), (324, _E256), (640, _E256)):
    _g(f"N{_N}-{'default' if not _env else '-'.join(f'{k[8:].lower()}{v}' for k, v in _env.items())}", M=130, N=_N, K=128, bias=True, env=_env)

# ---- K: 8; K % 64 != 0 (global_load_lds staging, the K tail); one K tile against use_8p(); nit8 on both sides of min_ktiles_192; packed taps ----
for _K in (8, 72, 120, 64, 128, 136):
    _g(f"g128x64-K{_K}", M=130, N=64, K=_K, bias=True)
    _g(f"big-tile-K{_K}", M=260, N=320, K=_K, bias=True, env=_E256)               # K % 64 != 0 or one tile: gemm_kernel<256,320>; else the 8-phase kernel
for _K in (192, 256):
    _g(f"8p192-mink-K{_K}", M=200, N=320, K=_K, bias=True, env=_E192)             # nit8 = 3 | 4 against ME_GEMM_192_MINK = 4
    _g(f"8p128-mink-K{_K}", M=200, N=320, K=_K, bias=True, env=_E128)
_g("default-M200-K256", M=200, N=320, K=256, bias=True)                            # the twin of 8p192-mink-K256 / 8p128-mink-K256 under the default thresholds
_g("8p192-mink2-K128", M=200, N=320, K=128, bias=True, env={"ME_GEMM_8P_192": 1, "ME_GEMM_192_MINK": 2})
_g("8p192-mink3-K128", M=200, N=320, K=128, bias=True, env={"ME_GEMM_8P_192": 1, "ME_GEMM_192_MINK": 3})
_g("8p256-off-K128", M=260, N=320, K=128, bias=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_8P": 0}, sel=2, pieces=(259,), twice=True)
_g("8p256-min3-K128", M=260, N=320, K=128, bias=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_8P": 3})
_g("8p256-min3-K192", M=260, N=320, K=192, bias=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_8P": 3})
for _K in (8, 16, 24, 32):
    _g(f"conv-packed-K{_K}", N=64, K=_K, bias=True, **_conv(3, 5, 7))
    _g(f"conv-packed-big-tile-K{_K}", N=320, K=_K, env=_E256, **_conv(3, 10, 13))
_g("tconv-K8", M=2 * 5 * 9, N=64, K=8, tconv=(5, 9, 5))
_g("tconv-K72-big-tile", M=2 * 5 * 30, N=320, K=72, tconv=(5, 30, 5), env=_E256)

# ---- split-K (csrc/gemm.hip:1605): nit 31 | 32; S = 2, 3, 4; blocks against ME_GEMM_SPLITK; scratch too small / misaligned; N < 1280 ----
_g("splitk-nit31", M=128, N=1280, K=31 * 64, bias=True)
_g("splitk-nit32-S4", M=128, N=1280, K=2048, bias=True, twice=True, sel=2)
_g("splitk-S3", M=1536, N=1280, K=2048, bias=True)                # 12 x 20 tiles of 128 x 64 = 240 blocks -> 3
_g("splitk-S2", M=2048, N=1280, K=2048, bias=True)                # 320 blocks -> 2
_g("splitk-blocks399", M=19 * 128, N=21 * 64, K=2048, env={"ME_GEMM_N64_BELOW": 1 << 30})      # 19 x 21 tiles of 128 x 64 against the default 400: split in two
_g("splitk-blocks400", M=20 * 128, N=1280, K=2048, env={"ME_GEMM_N64_BELOW": 1 << 30})         # 20 x 20: whole
_g("splitk-below-threshold", M=128, N=1280, K=2048, bias=True, env={"ME_GEMM_SPLITK": 21})       # 20 blocks < 21: split
_g("splitk-at-threshold", M=128, N=1280, K=2048, bias=True, env={"ME_GEMM_SPLITK": 20})          # 20 blocks >= 20: whole
_g("splitk-off", M=128, N=1280, K=2048, bias=True, env={"ME_GEMM_SPLITK": 0})
_g("splitk-work-short", M=128, N=1280, K=2048, bias=True, work="short")
_g("splitk-work-misaligned", M=128, N=1280, K=2048, bias=True, work="misaligned")
_g("splitk-N1216-never", M=128, N=1216, K=2048, bias=True)
_g("splitk-conv-nit36", N=1280, K=256, bias=True, **_conv(2, 8, 8))
_g("splitk-tconv-nit33", M=2 * 4 * 16, N=1280, K=704, tconv=(4, 16, 4))
_g("splitk-terms", M=130, N=1280, K=2048, bias=True, rowvec=50, res=True, res_rows=96, res2=True, alpha=0.5)
_g("splitk-act2", M=130, N=1280, K=2048, bias=True, rowvec=50, act=2, res=True)
_g("splitk-128x128", M=130, N=1280, K=2048, bias=True, env={"ME_GEMM_N64_BELOW": 0}, twice=True, sel=2)
_g("splitk-128x160", M=130, N=1440, K=2048, bias=True, twice=True, sel=2)
_g("splitk-256x320", M=260, N=1280, K=2048, bias=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_8P": 0}, twice=True, sel=2)
_g("splitk-m-off-never", M=130, N=1280, K=2048, bias=True, pieces=(129,), pieces_only=True)       # rows [0, 129) split (m_off = 0), row 129 alone does not
_g("splitk-geglu-never", M=130, N=1280, K=2048, bias=True, geglu=True)

# ---- the epilogue (csrc/gemm.hip:1793 launch_gemm8p: row pass of term sets 0, 2, 4, 6, 12, else direct) on the 8-phase kernel, the 128-row kernel's own ----
_TERMS = {0: {}, 2: dict(rowvec=77), 4: dict(res=True), 6: dict(rowvec=77, res=True), 12: dict(res=True, res2=True), 8: dict(res2=True), 10: dict(rowvec=77, res2=True),
          14: dict(rowvec=77, res=True, res2=True)}
for _f, _t in _TERMS.items():
    _g(f"epi-8p256-f{_f}", M=300, N=320, K=128, bias=True, env=_E256, **_t)
    _g(f"epi-8p192-f{_f}", M=300, N=640, K=256, bias=True, env=_E192, **_t)
    _g(f"epi-g128x64-f{_f}", M=300, N=320, K=72, bias=_f != 0, **_t)
for _act in (1, 2):
    _g(f"epi-8p256-act{_act}", M=300, N=320, K=128, bias=True, rowvec=77, res=True, act=_act, env=_E256)
    _g(f"epi-g128x64-act{_act}", M=300, N=64, K=128, bias=True, rowvec=77, res=True, res2=True, act=_act)
_g("epi-8p256-rowepi-off", M=300, N=320, K=128, bias=True, rowvec=77, res=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_ROWEPI": 0})
_g("epi-8p256-ldc-odd", M=300, N=320, K=128, bias=True, res=True, c_pad=4, env=_E256)          # ldc % 8 != 0
_g("epi-8p256-c-8-byte", M=300, N=320, K=128, bias=True, res=True, c_off=4, env=_E256)          # C 8-byte, not 16-byte aligned
_g("epi-8p256-res-8-byte", M=300, N=320, K=128, bias=True, res=True, res_off=4, env=_E256)
_g("epi-8p256-rpv-1", M=300, N=320, K=128, rowvec=1, env=_E256)
_g("epi-8p256-rpv-255", M=513, N=320, K=128, rowvec=255, env=_E256)
_g("epi-8p256-rpv-257", M=513, N=320, K=128, rowvec=257, env=_E256)
_g("epi-8p256-res-rows-96", M=300, N=320, K=128, res=True, res_rows=96, env=_E256)
_g("epi-8p256-res-rows-1", M=300, N=320, K=128, res=True, res_rows=1, res2=True, res2_rows=299, env=_E256)
_g("epi-8p256-alpha", M=300, N=320, K=128, bias=True, res=True, alpha=0.37, env=_E256)
_g("epi-g128x64-alpha", M=130, N=64, K=128, bias=True, res=True, alpha=-1.7)
_g("epi-8p256-out-aliases-res", M=300, N=320, K=128, bias=True, res="alias", env=_E256)
_g("epi-g128x64-out-aliases-res", M=130, N=64, K=128, bias=True, res="alias")
_g("epi-g256-out-aliases-res2", M=300, N=320, K=64, bias=True, res=True, res2="alias", env=_E256)
_g("epi-8p256-geglu-c-8-byte", M=300, N=256, K=128, bias=True, geglu=True, c_off=4, env={"ME_GEMM_GEGLU_MIN": 0})
_g("epi-8p256-geglu-rowepi-off", M=300, N=256, K=128, bias=True, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0, "ME_GEMM_ROWEPI": 0})

# ---- convolution geometry (csrc/gemm.hip gather): image boundaries inside a row tile, H = 1, W = 1, stride 2 on odd sizes, pad0, ups = 1 | 3, tconv chunks ----
_g("conv-5x7-images-in-a-tile", N=64, K=64, bias=True, **_conv(9, 5, 7))
_g("conv-5x7-big-tile", N=320, K=64, bias=True, env=_E256, **_conv(9, 5, 7))
_g("conv-H1", N=64, K=64, **_conv(3, 1, 40))
_g("conv-W1", N=64, K=64, **_conv(3, 40, 1))
_g("conv-1x1", N=64, K=64, **_conv(7, 1, 1))
_g("conv-s2-odd", N=64, K=64, bias=True, **_conv(3, 7, 9, stride=2))
_g("conv-s2-odd-big-tile", N=320, K=64, env=_E256, **_conv(5, 7, 9, stride=2))
_g("conv-s2-pad0", N=64, K=64, bias=True, **_conv(3, 8, 10, stride=2, pad0=1))
_g("conv-s2-pad0-odd", N=320, K=64, env=_E256, **_conv(3, 7, 9, stride=2, pad0=1))
_g("conv-s1-pad0", N=64, K=64, **_conv(2, 6, 5, pad0=1))
for _u in (1, 3):
    _g(f"conv-ups{_u}-128x64", N=64, K=64, bias=True, sel=2 if _u == 3 else 0, twice=_u == 3, **_conv(4, 5, 7, ups=_u))
    _g(f"conv-ups{_u}-8p256", N=320, K=64, bias=True, env=_E256, sel=2 if _u == 3 else 0, **_conv(4, 5, 7, ups=_u))
    _g(f"conv-ups{_u}-8p192", N=320, K=128, bias=True, env=_E192, **_conv(2, 6, 9, ups=_u))
    _g(f"conv-ups{_u}-g256", N=320, K=64, bias=True, rowvec=140, res=True, env={"ME_GEMM_BIG_MIN": 0, "ME_GEMM_8P": 0}, **_conv(4, 5, 7, ups=_u))
    _g(f"conv-ups{_u}-K72", N=128, K=72, bias=True, act=2, res=True, env={"ME_GEMM_N64_BELOW": 0}, **_conv(2, 3, 5, ups=_u))
    _g(f"conv-ups{_u}-128x160", N=160, K=64, bias=True, **_conv(2, 5, 7, ups=_u))
    _g(f"conv-ups{_u}-1x1-image", N=64, K=64, **_conv(5, 1, 1, ups=_u))
_g("conv-ups3-8p256-terms", N=320, K=64, bias=True, rowvec=140, res=True, env=_E256, **_conv(4, 5, 7, ups=3))     # terms: off the row pass (direct epilogue)
_g("tconv-first-last-frame-of-chunks", M=2 * 12 * 7, N=64, K=64, bias=True, tconv=(12, 7, 4))
_g("tconv-chunk-1", M=2 * 6 * 7, N=64, K=64, tconv=(6, 7, 1))
_g("tconv-sharded-middle", M=2 * 4 * 9, N=64, K=64, bias=True, tconv=(4, 9, 8, 2, 8, "prev", "next"))       # frames 2..5 of 8, chunk 8: both halos read
_g("tconv-sharded-first", M=2 * 4 * 9, N=64, K=64, tconv=(4, 9, 4, 0, 8, "none", "next"))                    # chunk 4 ends with the shard: the next halo is NOT read
_g("tconv-sharded-last-big-tile", M=2 * 3 * 50, N=320, K=64, env=_E256, tconv=(3, 50, 8, 5, 8, "prev", "none"))
_g("tconv-sharded-chunk-straddles", M=1 * 4 * 9, N=64, K=64, tconv=(4, 9, 4, 2, 8, "prev", "next"))          # frames 2..5: chunk boundary between 3 and 4
_g("conv-halo-512-images", prod=True, N=320, K=64, bias=True, sel=2, **_conv(512, 16, 16))

# ---- head-major second output, the LayerNorm fold (fused on the 8-phase kernels, on the 128-row kernels), ln_out (fused | me_ln_stats appended) ----
_g("c2-8p256-qkv", M=300, N=960, K=128, head_major=(320, 40), env=_E256)
_g("c2-8p256-all-panels", M=300, N=960, K=128, head_major=(0, 80), env=_E256)
_g("c2-g128x64-col0-80", M=130, N=320, K=72, head_major=(80, 40), bias=True)
_g("c2-g128x160-all-panels", M=130, N=480, K=128, head_major=(0, 160))
for _K in (320, 640, 960, 1280, 128):
    _g(f"ln-8p256-K{_K}", M=300, N=320, K=_K, ln=True, env=_E256)
    _g(f"ln-g128x64-K{_K}", M=130, N=64, K=_K, ln=True)
_g("ln-8p256-geglu", M=300, N=256, K=320, ln=True, geglu=True, env={"ME_GEMM_GEGLU_MIN": 0})
_g("ln-8p192-head-major", M=200, N=960, K=640, ln=True, head_major=(0, 40), env=_E192)
_g("ln-g128x64-glds-K328", M=130, N=64, K=328, ln=True)
_g("ln-large-mean", M=130, N=320, K=640, ln=True, mean=8.0, env=_E256)
for _n, _kw in (("8p256", dict(M=300, N=320, K=128, env=_E256)), ("8p256-N640-res", dict(M=300, N=640, K=128, res=True, env=_E256)), ("8p192", dict(M=200, N=320, K=256, env=_E192)),
                ("8p256-direct-f8", dict(M=300, N=320, K=128, res2=True, env=_E256)), ("g128x64", dict(M=130, N=64, K=128)), ("g128x64-N320", dict(M=130, N=320, K=72)),
                ("g256-one-k-tile", dict(M=300, N=320, K=64, env=_E256)), ("ups3", dict(N=320, K=64, env=_E256, **_conv(2, 5, 7, ups=3)))):
    _g(f"lnout-{_n}", bias=True, ln_out=True, **_kw)

GEMM_PAIRS = [
    ("ME_GEMM_BIG_MIN", "gemm-N320-default", "gemm-N320-big_min0"), ("ME_GEMM_8P", "gemm-8p256-off-K128", "gemm-big-tile-K128"),
    ("ME_GEMM_8P", "gemm-8p256-min3-K128", "gemm-big-tile-K128"), ("K against ME_GEMM_8P", "gemm-8p256-min3-K128", "gemm-8p256-min3-K192"),
    ("K against ME_GEMM_8P", "gemm-big-tile-K64", "gemm-big-tile-K128"),
    ("ME_GEMM_8P_192", "gemm-default-M200-K256", "gemm-8p192-mink-K256"), ("ME_GEMM_8P_128", "gemm-default-M200-K256", "gemm-8p128-mink-K256"),
    ("ME_GEMM_ROWEPI", "gemm-epi-8p256-rowepi-off", "gemm-epi-8p256-f6"),       # (the same kernel NAME: the pair differs in gemm_epilogue, row6 against direct)
    ("ME_GEMM_192_MINK", "gemm-8p192-mink3-K128", "gemm-8p192-mink2-K128"), ("K against ME_GEMM_192_MINK", "gemm-8p192-mink-K192", "gemm-8p192-mink-K256"),
    ("K against ME_GEMM_192_MINK", "gemm-8p128-mink-K192", "gemm-8p128-mink-K256"),
    ("ME_GEMM_N64_BELOW", "gemm-N128-n64_below0", "gemm-N128-default"), ("ME_GEMM_N64_BELOW", "gemm-N320-n64_below0", "gemm-N320-default"),
    ("ME_GEMM_SPLITK", "gemm-splitk-at-threshold", "gemm-splitk-below-threshold"), ("ME_GEMM_SPLITK", "gemm-splitk-off", "gemm-splitk-nit32-S4"),
    ("K against nit >= 32", "gemm-splitk-nit31", "gemm-splitk-nit32-S4"), ("N against 1280", "gemm-splitk-N1216-never", "gemm-splitk-nit32-S4"),
    ("ME_GEMM_GEGLU_MIN", "gemm-g128x64-geglu-default", "gemm-8p256-geglu-forced"), ("N % 320", "gemm-N316-big_min0", "gemm-N320-big_min0"), ("N % 320", "gemm-N324-big_min0", "gemm-N320-big_min0"),
    ("N % 64", "gemm-N68-default", "gemm-N64-default"), ("N % 128", "gemm-N192-n64_below0", "gemm-N128-n64_below0"), ("N % 160", "gemm-N164-default", "gemm-N160-default"),
    ("N % 256", "gemm-geglu-N288-forced", "gemm-8p256-geglu-forced"),
]
PAIRS += GEMM_PAIRS


# ---- attention (csrc/attn.hip me_attn): every attn2_kernel / attn_kernel instantiation at its query-block and key-stage edges ----
def _attn_args(p):
    modes = {m for r in p.get("modes", ()) for m in r}
    return dict(dh=p["dh"], nq=p["nq"], nk=p["nk"], nseg=max(len(r) for r in p["table"]), general_dual=bool(modes & {1, 2}), vsum=3 in modes and not modes & {1, 2},
                o_al=not p.get("o_off") and not p.get("o_pad"))


def _a(id_, twice=False, **p):
    p.setdefault("heads", 8)
    p.setdefault("table", [[0], [1]])
    p.setdefault("n_kv", 1 + max(k for r in p["table"] for k in r))
    CASES.append(Case(id=f"attn-{id_}", entry="attention", p=p, path=attn_target(_attn_args(p), p.get("env")), twice=twice))


_NK_CLASSIC = (1, 15, 16, 17, 63, 64, 65, 80, 81, 255)
_PC = [[0, -1], [0, 1], [1, 2]]
_heads = (1, 5, 8)
# (label, dh, nq values that select the kernel, env): the classic / fold pair of every (dh, query-block form)
_FORMS = (("40-4w", 40, (1, 127, 128, 129, 255), None), ("40-8w", 40, (256, 257, 511), None), ("40-16w", 40, (512, 513, 1023), None),
          ("80-qt2-4w", 80, (1, 127), None), ("80-8w", 80, (128, 129, 255), None), ("80-8w-256", 80, (256, 257), {"ME_ATTN_80_QT2": 0}), ("80-qt2-8w", 80, (256, 257, 511), None),
          ("160-4w", 160, (1, 63, 64, 65, 255, 256), None))
for _lab, _dh, _nqs, _env in _FORMS:
    for _i, _nq in enumerate(_nqs):                        # nq edges at one ragged key count below and one above the fold threshold
        _a(f"{_lab}-nq{_nq}-nk70x1", dh=_dh, nq=_nq, nk=70, heads=_heads[_i % 3], table=[[0], [1]], env=dict(_env or {}, ME_ATTN_KVRES=0), lse=True)
        if _dh != 160:
            _a(f"{_lab}-nq{_nq}-nk257", dh=_dh, nq=_nq, nk=257, heads=_heads[(_i + 1) % 3], table=[[0], [1]], env=_env, lse=True)
    _nq = _nqs[1] if len(_nqs) > 1 else _nqs[0]
    if _lab in ("40-16w", "80-qt2-8w"):                    # fold-only forms (nq >= 512 at dh 40 is the 8-wave classic kernel below nk = 256)
        continue
    for _i, _nk in enumerate(_NK_CLASSIC):                 # key edges of the classic sweep
        _a(f"{_lab}-nk{_nk}-nq{_nq}", dh=_dh, nq=_nq, nk=_nk, heads=_heads[_i % 3], table=[[0, 1], [1, -1]], env=dict(_env or {}, ME_ATTN_KVRES=0))
for _lab, _dh, _nq, _env in (("40-4w", 40, 130, None), ("40-8w", 40, 300, None), ("40-16w", 40, 520, None), ("80-qt2-4w", 80, 100, None), ("80-8w", 80, 130, None),
                             ("80-8w-256", 80, 300, {"ME_ATTN_80_QT2": 0}), ("80-qt2-8w", 80, 300, None)):
    _stage = attn_geometry(attn_target(dict(dh=_dh, nq=_nq, nk=256), _env))[1]
    for _i, _nk in enumerate(sorted({256, 257, 256 + _stage - 1, 256 + _stage, 256 + _stage + 1, 256 + 2 * _stage - 1, 319, 320, 321})):
        _a(f"{_lab}-fold-nk{_nk}-nq{_nq}", dh=_dh, nq=_nq, nk=_nk, heads=_heads[_i % 3], table=[[0], [1]], env=_env, lse=_i % 2 == 0)
_a("160-nk256", dh=160, nq=70, nk=256, heads=5)
_a("160-nk257-two-seg", dh=160, nq=130, nk=257, heads=1, table=[[0, 1], [1, -1]])
# keys resident across query blocks (64 < nk <= 80, one segment, O 16-byte aligned with ldo % 8 == 0): both sides of nk, of nq, of every way out
for _dh, _nqs in ((40, (511, 512, 513, 767, 1025)), (80, (255, 256, 257, 383, 385)), (160, (255, 256, 257, 383, 385))):
    for _i, _nq in enumerate(_nqs):
        _a(f"kvres-dh{_dh}-nq{_nq}-nk77", dh=_dh, nq=_nq, nk=77, heads=(8, 8, 5, 1, 5)[_i], table=[[0], [0], [1]], lse=True)
    _nq = _nqs[1]
    for _nk in (64, 65, 77, 80, 81):
        _a(f"kvres-dh{_dh}-nk{_nk}", dh=_dh, nq=_nq, nk=_nk, table=[[0], [1]])
    _a(f"kvres-dh{_dh}-qpb2", dh=_dh, nq=3 * _nq + 5, nk=77, table=[[0], [1]], env={"ME_ATTN_KVRES": 2}, twice=True)       # two query blocks per block, not a divisor
    _a(f"kvres-dh{_dh}-off", dh=_dh, nq=_nq, nk=77, table=[[0], [1]], env={"ME_ATTN_KVRES": 0})
    _a(f"kvres-dh{_dh}-two-seg", dh=_dh, nq=_nq, nk=77, table=[[0, 1], [1, -1]])
    _a(f"kvres-dh{_dh}-o-8-byte", dh=_dh, nq=_nq, nk=77, table=[[0], [1]], o_off=4)
    _a(f"kvres-dh{_dh}-ldo-odd", dh=_dh, nq=_nq, nk=77, table=[[0], [1]], o_pad=4)
    _a(f"kvres-dh{_dh}-q-items", dh=_dh, nq=_nq, nk=77, table=[[0], [1], [1], [0]], q_items=2, heads=5)
# segment lists: 1, 2 and 3 segments, a skipped segment, mixed modes, more kv items than query items, strided Q and O, head-major Q / K / V, item_order
_a("nseg3-ragged", dh=40, nq=70, nk=33, table=[[0, 1, 2], [1, -1, -1], [2, 0, -1], [3, 3, 3]])
_a("nseg2-skip-dh80", dh=80, nq=130, nk=50, heads=5, table=[[1, -1], [0, 1], [2, -1], [2, 0]])
_a("nseg3-fold-dh40", dh=40, nq=260, nk=257, heads=1, table=[[0, 1, 2], [2, -1, -1]])
_a("nseg3-dh160", dh=160, nq=65, nk=65, heads=5, table=[[0, 1, 2], [2, 1, -1]])
_a("n-kv-gt-items", dh=40, nq=64, nk=72, table=[[5, 0], [2, -1]], n_kv=6, lse=True)
_a("q-items", dh=80, nq=100, nk=90, table=[[0], [1], [2], [0]], q_items=2, lse=True)
_a("strided-q-o", dh=40, nq=130, nk=100, table=_PC, q_pad=16, o_pad=24, scale=0.2)
_a("fused-qkv-views", dh=80, nq=96, nk=96, table=_PC, fused=True)
for _dh, _nq, _nk in ((40, 130, 100), (80, 260, 257), (160, 70, 77), (40, 520, 300)):
    _a(f"head-major-kv-dh{_dh}-nq{_nq}", dh=_dh, nq=_nq, nk=_nk, table=_PC, head_major="kv")
    _a(f"head-major-qkv-dh{_dh}-nq{_nq}", dh=_dh, nq=_nq, nk=_nk, table=_PC, head_major="qkv", heads=5)
_a("item-order-dh40", dh=40, nq=130, nk=100, table=[[0, 1], [1, 2], [2, 3], [3, 0], [0, 2]], item_order=[3, 0, 4, 1, 2])
_a("item-order-fold-dh80", dh=80, nq=260, nk=256, table=[[0, 1], [1, 2], [2, 0]], item_order=[2, 0, 1], heads=5)
# the dual modes: DUAL_BIN (+ 1 per key, the vsum pre-pass: 51 row lanes at heads * dh = 40, one at 2000, empty row splits below 16 keys), the general-dual kernels
for _dh, _heads_, _nq, _nk in ((40, 1, 70, 100), (80, 25, 20, 40), (40, 8, 130, 9), (40, 8, 300, 257), (80, 5, 260, 256), (160, 8, 70, 64), (40, 8, 520, 300)):
    _a(f"dual-bin-dh{_dh}-h{_heads_}-nq{_nq}-nk{_nk}", dh=_dh, heads=_heads_, nq=_nq, nk=_nk, table=[[0, 1], [1, 2], [2, -1]], modes=[[3, 0], [0, 3], [3, 0]], twice=_nk == 9)
_a("dual-bin-head-major-v", dh=40, nq=130, nk=77, table=[[0, 1], [1, 0]], modes=[[3, 0], [3, 3]], head_major="kv")
for _dh in (40, 80, 160):
    _bq = 64 if _dh == 160 else 128
    for _i, _nq in enumerate((1, _bq - 1, _bq, _bq + 1)):
        _a(f"general-dual-dh{_dh}-nq{_nq}", dh=_dh, nq=_nq, nk=(63, 64, 65, 130)[_i], heads=_heads[_i % 3], table=[[0, 1, 2], [1, 2, -1], [2, -1, -1]], modes=[[1, 2, 0], [2, 1, 0], [0, 0, 0]])
    _a(f"general-dual-dh{_dh}-prev-clamp", dh=_dh, nq=40, nk=17, heads=8, table=[[0], [1]], modes=[[2], [2]])
    _a(f"general-dual-dh{_dh}-head-major", dh=_dh, nq=70, nk=100, heads=5, table=[[0, 1], [1, 0]], modes=[[1, 0], [2, 1]], head_major="qkv")
# the fixed-offset softmax's fallback: a ragged last query block; padded zero queries must not trip it (flat), saturating real ones must (peaked)
_a("fold-ragged-flat", dh=40, nq=257, nk=640, table=[[0], [1]], fallback=False)
_a("fold-ragged-peaked", dh=40, nq=257, nk=640, table=[[0], [1]], peaked=15.0, fallback=True, lse=True)
_a("fold-ragged-peaked-dh80", dh=80, nq=129, nk=640, table=[[0], [1]], peaked=15.0, fallback=True)

ATTN_PAIRS = [
    ("ME_ATTN_80_QT2", "attn-80-8w-256-nq256-nk257", "attn-80-qt2-8w-nq256-nk257"),
    ("nk against 64 (kvres)", "attn-kvres-dh80-nk64", "attn-kvres-dh80-nk65"), ("nk against 80 (kvres)", "attn-kvres-dh160-nk81", "attn-kvres-dh160-nk80"),
    ("nq against 512 (kvres, dh 40)", "attn-kvres-dh40-nq511-nk77", "attn-kvres-dh40-nq512-nk77"),
    ("nq against 256 (kvres, dh 80)", "attn-kvres-dh80-nq255-nk77", "attn-kvres-dh80-nq256-nk77"),
    ("nq against 256 (kvres, dh 160)", "attn-kvres-dh160-nq255-nk77", "attn-kvres-dh160-nq256-nk77"),
]
for _dh in (40, 80, 160):
    ATTN_PAIRS += [("ME_ATTN_KVRES", f"attn-kvres-dh{_dh}-off", f"attn-kvres-dh{_dh}-nk77"), ("O alignment (kvres)", f"attn-kvres-dh{_dh}-o-8-byte", f"attn-kvres-dh{_dh}-nk77"),
                   ("ldo % 8 (kvres)", f"attn-kvres-dh{_dh}-ldo-odd", f"attn-kvres-dh{_dh}-nk77"), ("nseg (kvres)", f"attn-kvres-dh{_dh}-two-seg", f"attn-kvres-dh{_dh}-nk77")]
# (dh, nk, nq below, nq at, env): the selecting thresholds on nq, classic and fold; then nk across 256 at every (dh, query-block form)
for _dh, _nk, _lo, _hi, _env in ((80, 70, 127, 128, {"ME_ATTN_KVRES": 0}), (40, 70, 255, 256, {"ME_ATTN_KVRES": 0}), (40, 257, 255, 256, None), (40, 257, 511, 512, None),
                                 (80, 257, 127, 128, None), (80, 257, 255, 256, None), (80, 257, 127, 128, {"ME_ATTN_80_QT2": 0})):
    _tag = "" if not _env else "-" + "-".join(f"{k[8:].lower()}{v}" for k, v in _env.items())
    for _nq in (_lo, _hi):
        _a(f"pair-dh{_dh}-nq{_nq}-nk{_nk}{_tag}", dh=_dh, nq=_nq, nk=_nk, table=[[0], [1]], env=_env)
    ATTN_PAIRS.append((f"nq against {_hi} (dh {_dh})", f"attn-pair-dh{_dh}-nq{_lo}-nk{_nk}{_tag}", f"attn-pair-dh{_dh}-nq{_hi}-nk{_nk}{_tag}"))
for _dh, _nq in ((40, 130), (40, 300), (80, 100), (80, 130), (80, 300)):
    for _nk in (255, 256):
        _a(f"pair-dh{_dh}-nq{_nq}-nk{_nk}", dh=_dh, nq=_nq, nk=_nk, table=[[0, 1], [1, -1]])
    ATTN_PAIRS.append(("nk against 256", f"attn-pair-dh{_dh}-nq{_nq}-nk255", f"attn-pair-dh{_dh}-nq{_nq}-nk256"))
PAIRS += ATTN_PAIRS


# ---- temporal attention (csrc/tattn.hip): the MFMA form (KP = 32 | 64) at every head dim, the per-thread form through dh = 8 / 32 / 320 ----
def _t(id_, **p):
    p.setdefault("npix", 3)
    p.setdefault("batch", 2)
    CASES.append(Case(id=f"tattn-{id_}", entry="temporal_attention", p=p, path=tattn_target(p)))


TATTN_MFMA_FRAMES = (1, 7, 8, 31, 32, 33, 48, 64)
TATTN_THREAD_FRAMES = (8, 16, 24, 32, 40, 48)
for _F in TATTN_MFMA_FRAMES:
    for _dh in (40, 80, 160):
        _t(f"mfma-F{_F}-dh{_dh}", frames=_F, dh=_dh, heads=320 // _dh * (2 if _F == 8 else 1))
for _dh in (40, 80, 160):
    _t(f"mfma-npix1-batch8-dh{_dh}", frames=24, dh=_dh, heads=320 // _dh, npix=1, batch=8, kv_map=[1, 0, 3, 2, 7, 7, 0, 5])
    _t(f"mfma-q-frames-dh{_dh}", frames=24, dh=_dh, heads=320 // _dh, q_frames=5, q_frame0=7, kv_parts=3)
    _t(f"mfma-q-frames-last-dh{_dh}", frames=48, dh=_dh, heads=320 // _dh, q_frames=16, q_frame0=32, kv_parts=1, batch=1)
    _t(f"mfma-pixel-sharded-dh{_dh}", frames=24, dh=_dh, heads=320 // _dh, kv_parts=4, q_parts=4, npix=5)
    _t(f"mfma-strided-dh{_dh}", frames=16, dh=_dh, heads=320 // _dh, fused=True, scale=0.2)
for _dh in (32, 320):
    for _F in TATTN_THREAD_FRAMES:
        _t(f"thread-F{_F}-dh{_dh}", frames=_F, dh=_dh, heads=320 // _dh)
_t("thread-F8-dh8", frames=8, dh=8, heads=40)
_t("thread-F16-dh8-q-frames", frames=16, dh=8, heads=40, q_frames=12, q_frame0=4, batch=1)             # 40 x 12 = 480 threads: inside the 512
_t("thread-npix1-batch8", frames=16, dh=32, heads=20, npix=1, batch=8, kv_map=[1, 0, 3, 2, 7, 7, 0, 5])
_t("thread-q-frames", frames=24, dh=32, heads=10, q_frames=5, q_frame0=7, kv_parts=3)
_t("thread-pixel-sharded", frames=24, dh=320, heads=2, kv_parts=4, q_parts=4, npix=5)
TATTN_REFUSED_THREADS = dict(frames=16, dh=8, heads=40, npix=1, batch=1)           # 40 x 16 = 640 threads per block


# ---- the smaller families at the chunk edges of bwd_cases.gn_fwd_scratch_bytes (csrc/norm.hip gn_chunks), the LayerNorm half-wave kernel, softmax ----
def _s(id_, entry, twice=False, **p):
    CASES.append(Case(id=id_, entry=entry, p=p, twice=twice))


for _rpg, _nsg, _C in ((1, 3, 320), (24, 2, 320), (25, 2, 640), (383, 2, 320), (385, 1, 320), (4095, 1, 320), (4096, 2, 320), (4097, 1, 320), (6145, 1, 64), (98305, 1, 32),
                       (97, 3, 960), (50, 3, 1920), (33, 8, 2560), (64, 2, 1280)):
    # chunk_rows = ceil(rpg / 16) in [24, 256] up to 4096 rows, ceil(rpg / 256) in [24, 384] beyond: 25 -> a last chunk of ONE row; 385 -> 25-row chunks, the
    # last holds 10; 4096 -> 256 (the upper clamp met exactly); 4097 -> 24 (the lower clamp of the large form); 98305 -> 384 + a last chunk of one row
    _s(f"gn-rpg{_rpg}-nsg{_nsg}-C{_C}", "groupnorm", twice=_rpg in (4096, 4097), rpg=_rpg, nsg=_nsg, C=_C, silu=_rpg % 2 == 1)
    if _rpg in (25, 4096, 4097, 97):
        _s(f"gn-split-rpg{_rpg}-nsg{_nsg}-C{_C}", "groupnorm", rpg=_rpg, nsg=_nsg, C=_C, silu=_rpg % 2 == 0, split=2)
_s("gn-large-mean", "groupnorm", rpg=2048, nsg=2, C=320, silu=True, mean=100.0, spread=1.0)
_s("gn-strided", "groupnorm", rpg=50, nsg=3, C=640, silu=False, x_pad=8)
for _rows, _C in ((1, 320), (3, 8), (5, 512), (4, 520), (7, 1024), (5, 1032), (9, 1536), (4095, 320), (4096, 320), (4097, 320), (4113, 320), (130, 640), (77, 1280)):
    _s(f"ln-rows{_rows}-C{_C}", "layernorm", rows=_rows, C=_C, x_pad=8 if _rows % 2 else 0)
_s("ln-large-mean", "layernorm", rows=130, C=640, mean=100.0, spread=1.0)
for _rows, _cols in ((1, 8), (3, 72), (5, 1024), (4, 1032), (130, 4096), (3, 4104), (9, 8192)):
    _s(f"softmax-{_rows}x{_cols}", "softmax_rows", rows=_rows, cols=_cols, pad=0 if _cols == 1024 else 8, inplace=_cols == 72)

BY_ID = {c.id: c for c in CASES}
ENTRIES = sorted({c.entry for c in CASES})


def case_counts() -> Dict[str, int]:
    out: Dict[str, int] = {}
    for c in CASES:
        out[c.entry] = out.get(c.entry, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------- seeded input builders (CPU tensors)
def _gen(case):
    # a convolution over the nearest-2x upsample runs on THE SAME DATA in both of its forms: the ups = 3 case draws what its ups = 1 twin draws (and folds its weights)
    twin = case.entry == "gemm" and case.p.get("conv") and case.p["conv"][5] == 3
    return torch.Generator().manual_seed(seed_of(case.id.replace("ups3", "ups1") if twin else case.id))


def ups_twin(case):
    """The ups = 1 case on the same data as an ups = 3 case (None where the table holds none)."""
    return BY_ID.get(case.id.replace("ups3", "ups1")) if "ups3" in case.id else None


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def fold_ups(w9: torch.Tensor) -> torch.Tensor:
    """[N, 9, K] -> the folded [N, 16, K] of ups = 3 (include/motioned.h): tap (ty, tx) of parity (py, px) holds the sum of the 3 x 3 taps that land on
    low-resolution pixel (y + py - 1 + ty, x + px - 1 + tx); summed in fp32, rounded once."""
    N, _, K = w9.shape
    w16 = torch.zeros((N, 16, K), dtype=torch.float32)
    t_of = lambda par, k: (par - 1 + k) // 2 - par + 1    # noqa: E731
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    w16[:, 4 * (2 * py + px) + 2 * t_of(py, ky) + t_of(px, kx)] += w9[:, 3 * ky + kx].float()
    return w16.half()


def gemm_rows_in(p) -> int:
    if p.get("conv"):
        Hin, Win, Hout, Wout = p["conv"][:4]
        return p["M"] // (Hout * Wout) * Hin * Win
    return p["M"]


def build(case) -> dict:
    """The CPU input tensors of a case, fp16 / fp32 as the HIP entry point takes them; views and guard bands are cut by the runner (tests/fwd_run.py)."""
    p, g, e = case.p, _gen(case), case.entry
    if e == "gemm":
        M, N, K = p["M"], p["N"], p["K"]
        conv, tconv = p.get("conv"), p.get("tconv")
        taps = 9 if conv else (3 if tconv else 1)
        rows_in = gemm_rows_in(p)
        halo = 0
        if tconv and len(tconv) > 3:
            halo = M // tconv[0]                                  # nb * npix rows per one-frame halo
        x = _randn(g, rows_in + 2 * halo, K) + p.get("mean", 0.0)
        x = torch.cat([x, torch.full((x.shape[0], 8), 7.0)], dim=1).half()          # ldx = K + 8: the padding columns hold a value that must not be read
        w = _randn(g, N, taps, K, scale=(taps * K) ** -0.5).half()
        if conv and conv[5] == 3:
            w = fold_ups(w)
        d = dict(x=x, w=w)
        n_out = N // 2 if p.get("geglu") else N
        if p.get("bias"):
            d["bias"] = _randn(g, N).half()
        if p.get("rowvec"):
            d["rowvec"] = _randn(g, (M + p["rowvec"] - 1) // p["rowvec"], N).half()
        if p.get("res"):
            d["res"] = _randn(g, p.get("res_rows") or M, n_out).half()
        if p.get("res2"):
            d["res2"] = _randn(g, p.get("res2_rows") or M, n_out).half()
        if p.get("ln"):
            xf = x[:, :K].double()
            P = K // 320 if K % 320 == 0 else 1
            t = xf.reshape(x.shape[0], P, K // P)
            d["ln_stats"] = torch.stack([t.sum(-1), (t * t).sum(-1)], dim=-1).permute(1, 0, 2).contiguous().float()
            d["ln_colsum"] = w[:, 0].float().sum(dim=1)
            d["ln_cvec"] = _randn(g, N)
        return d
    if e == "attention":
        dh, heads, nq, nk, n_kv = p["dh"], p["heads"], p["nq"], p["nk"], p["n_kv"]
        C, n_items = heads * dh, len(p["table"])
        nqi = p.get("q_items") or n_items
        q, k, v = _randn(g, nqi * nq, C, scale=0.7), _randn(g, n_kv * nk, C, scale=0.7), _randn(g, n_kv * nk, C)
        if p.get("peaked"):       # as bwd_cases: 32 keys of the last tiles sit p["peaked"] nats above the typical logit of every REAL query (padded rows are zero queries)
            q, k = q * (0.5 / 0.7), k * (0.5 / 0.7)
            scale = dh ** -0.5
            for it in range(n_items):
                for h in range(heads):
                    qs = q[it * nq:(it + 1) * nq, h * dh:(h + 1) * dh]
                    dvec = qs.mean(0)
                    dvec = dvec / dvec.norm()
                    qs += dvec * 3.0
                    k0 = p["table"][it][0] * nk + nk - 102
                    k[k0:k0 + 32, h * dh:(h + 1) * dh] += dvec * (p["peaked"] / (3.0 * scale))
        nseg = max(len(r) for r in p["table"])
        tab = torch.tensor([list(r) + [-1] * (nseg - len(r)) for r in p["table"]], dtype=torch.int32)
        modes = torch.tensor([list(r) + [0] * (nseg - len(r)) for r in p["modes"]], dtype=torch.int32) if p.get("modes") else torch.zeros_like(tab)
        d = dict(q=q.half(), k=k.half(), v=v.half(), seg_item=tab, seg_mode=modes)
        if p.get("modes") and {m for r in p["modes"] for m in r} & {1, 2}:
            d["mask"] = torch.rand(8, nk, generator=g).half()
        return d
    if e == "temporal_attention":
        C = p["heads"] * p["dh"]
        rows_kv = p["batch"] * p["frames"] * p["npix"]
        rows_q = p["batch"] * (p.get("q_frames") or p["frames"]) * p["npix"]
        return dict(q=_randn(g, rows_q, C, scale=0.7).half(), kv=_randn(g, rows_kv, 2 * C, scale=0.7).half())
    if e == "groupnorm":
        C, rows = p["C"], p["rpg"] * p["nsg"]
        x = _randn(g, rows, C) * p.get("spread", 1.5) + p.get("mean", 0.5)
        return dict(x=x.half(), gamma=(1 + 0.2 * _randn(g, C)).half(), beta=(0.2 * _randn(g, C)).half())
    if e == "layernorm":
        rows, C = p["rows"], p["C"]
        x = (_randn(g, rows, C) * p.get("spread", 2.0) + p.get("mean", 0.3)).half()
        return dict(x=x, gamma=(1 + 0.2 * _randn(g, C)).half(), beta=(0.2 * _randn(g, C)).half())
    if e == "softmax_rows":
        return dict(x=_randn(g, p["rows"], p["cols"], scale=4.0).half())
    raise KeyError(e)
