"""TEST INFRASTRUCTURE: the case table of the backward / training sweep (tests/test_bwd_sweep_cpu.py, tests/test_bwd_sweep_gpu.py).

Pure data and seeded input builders; nothing here imports the HIP side.  A case names its entry point (the ``motioneditor_amd.ops`` function), the
parameters its builder turns into tensors, and -- where the launch code names its kernel -- the kernel the case was written for (an fnmatch pattern
checked against ``me_last_kernel``).  The edges are derived from the launch code; the file and line are cited next to each family.

Tolerances are the ones the project already states per entry point (tests/test_kernels_gpu.py), restated here by name, and
tests/test_bwd_sweep_cpu.py asserts the fp32 emulation against the fp64 reference inside the same bound on every case, which shows the bound is reachable by
fp32 accumulation on these very inputs.  Where a case cannot be held to max-error / mean-magnitude it says so in its own entry:
  elementwise=   six cases (softmax_bwd_rows, which had no test and no bound before, and geglu-fp16-overflow) replace max / mean by a per-element limit
                 derived from the number formats; the derivation stands next to the entries and in elementwise_limit below.  rel-L2 stays the entry point's.
  zero=          gradients that are identically zero get the absolute bound of bwd_run.single_key_zero_bound.
  bound=         a wider (rel-L2, max / mean) for one case: measure the fp32 emulation's error against the fp64 reference on this CPU (the floor), allow four
                 times it, and write floor, factor and bound into the entry -- never a figure taken from what the kernel under test returned.  No case uses it.
AdamW is held to its entry point's bound on p, m and v alike; the fp64 reference takes the hyper-parameters as me_adamw's fp32 signature carries them."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

# ---------------------------------------------------------------------------------------------------------------- bounds (rel-L2, max-abs / mean-abs)
REL_L2, MAX_REL = 2e-3, 2e-2          # tests/test_kernels_gpu.py: fp16 storage, fp32 accumulation
BWD_REL, BWD_MAX = 4e-3, 6e-2         # test_attention_bwd_plain_segments / test_gemm_dw_and_bias_gradients: rel=4e-3, mx=6e-2
BOUNDS: Dict[str, Tuple[float, float]] = {
    "gemm_dx": (REL_L2, MAX_REL),                 # test_gemm_dx_matches_the_vjp_of_the_forward_emulation
    "gemm_dw": (BWD_REL, BWD_MAX),                # test_gemm_dw_and_bias_gradients
    "colsum_grad": (1e-4, 1e-3),                  # ... its colsum_grad line
    "geglu_bwd": (REL_L2, MAX_REL),               # test_geglu_bwd
    "layernorm_bwd": (REL_L2, MAX_REL),           # test_layernorm_bwd
    "layernorm_bwd_params.dgamma": (1e-3, 2e-2),  # test_relu_bwd_and_layernorm_param_gradients
    "layernorm_bwd_params.dbeta": (1e-4, 1e-3),
    "groupnorm_bwd": (REL_L2, MAX_REL),           # test_groupnorm_bwd
    "attention_bwd": (BWD_REL, BWD_MAX),          # test_attention_bwd_plain_segments
    "temporal_attention_bwd": (REL_L2, MAX_REL),  # test_temporal_attention_bwd
    "softmax_bwd_rows": (REL_L2, MAX_REL),        # fp16 in, fp16 out: the per-kernel rel-L2; per element elementwise="f16-out" instead of max / mean
    "relu_bwd": (0.0, 0.0),                       # a selection: exact (test_relu_bwd_and_layernorm_param_gradients uses torch.equal)
    "grad_acc.f32": (1e-6, 1e-2),                 # test_grad_acc_plain_strided_fp16_and_pooled
    "grad_acc.f16": (1e-3, 1e-2),
    "adamw": (1e-5, 1e-4),                        # test_adamw_kernel_matches_torch_optim
    "sumsq_absmax": (1e-5, 0.0),                  # test_sumsq_absmax_...: sum of squares to 1e-5, the maximum exact
    "mse_seed": (1e-6, 1e-5),                     # test_cast_kernels_and_mse_seed
    "cast_f16": (0.0, 0.0),                       # casts are exact
    "cast_rows_f16": (0.0, 0.0),
}


@dataclass
class Case:
    id: str
    entry: str
    p: dict
    path: Optional[str] = None       # fnmatch pattern of me_last_kernel after the launch, where the launch names its kernel
    prod: bool = False               # a production-size launch (the mutant search of the CPU file leaves these out)
    twice: bool = False              # the same call twice must be bitwise equal
    bound: Optional[Tuple[float, float]] = None
    elementwise: Optional[str] = None   # the per-element limit (elementwise_limit) that stands in for max / mean


def seed_of(case_id: str) -> int:
    return zlib.crc32(case_id.encode()) & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------------- launch geometry, restated
def dw_geometry(M: int, N: int, K: int) -> Tuple[int, int, str]:
    """csrc/train.hip:124 dw_geometry -> (splits, rows_per_split, the clamp that decided the split count)."""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    s, why = (1024 + tiles - 1) // tiles, "tiles"          # ~1024 blocks
    smax = (M + 4 * 32 - 1) // (4 * 32)                     # at least four 32-row stages per split
    if s > smax:
        s, why = smax, "stages"
    if s > 256:
        s, why = 256, "cap256"
    if s < 1:
        s = 1
    rps = (M + s - 1) // s
    rps = (rps + 31) // 32 * 32
    return (M + rps - 1) // rps, rps, why


def dw_work_bytes(M: int, N: int, K: int) -> int:
    return dw_geometry(M, N, K)[0] * N * K * 4 if min(M, N, K) > 0 else 0


def dw_edges(N: int, K: int, m_max: int, interior: int = 3):
    """Sweep M = 1 .. m_max and return the M on both sides of every point where the deciding clamp changes and where splits leaves 1, plus, of the points
    inside each regime where splits or rows_per_split changes, the first, the last and `interior` evenly spaced ones between them.  A SUB-SAMPLE: inside
    a regime there is one such point every 32 or 128 rows (hundreds per shape) and consecutive ones follow the same arithmetic; a swallowed split and a
    one-row last split have cases of their own."""
    picks, prev, changes = set(), None, {}
    for M in range(1, m_max + 1):
        cur = dw_geometry(M, N, K)
        if prev is not None:
            if cur[2] != prev[2] or (prev[0] == 1) != (cur[0] == 1):
                picks.update((M - 1, M))
            if cur[:2] != prev[:2]:
                changes.setdefault(cur[2], []).append(M)
        prev = cur
    for ms in changes.values():
        for i in range(interior + 2):
            M = ms[i * (len(ms) - 1) // (interior + 1)]
            picks.update((M - 1, M))
    return sorted(m for m in picks if 1 <= m <= m_max)


def gn_bwd_chunks(rows: int, rows_per_group: int) -> Tuple[int, int]:
    """csrc/bwd.hip gn_bwd_chunks -> (chunks, chunk_rows)."""
    nsg = rows // rows_per_group
    chunks = max(1, min(512, 1024 // nsg))
    chunk_rows = max(8, (rows_per_group + chunks - 1) // chunks)
    return (rows_per_group + chunk_rows - 1) // chunk_rows, chunk_rows


def gn_fwd_scratch_bytes(rows: int, rows_per_group: int, groups: int) -> int:
    """csrc/norm.hip me_groupnorm_scratch_bytes (the statistics pass the backward reuses)."""
    big = rows_per_group > 4096
    chunk_rows = (rows_per_group + (255 if big else 15)) // (256 if big else 16)
    chunk_rows = min(max(chunk_rows, 24), 384 if big else 256)
    chunks = (rows_per_group + chunk_rows - 1) // chunk_rows
    nsg = rows // rows_per_group
    return nsg * groups * 2 * 8 + chunks * nsg * groups * 16


def gn_bwd_scratch_bytes(rows: int, rows_per_group: int, groups: int) -> int:
    """csrc/bwd.hip me_groupnorm_bwd_scratch_bytes."""
    chunks, _ = gn_bwd_chunks(rows, rows_per_group)
    nsg = rows // rows_per_group
    return (gn_fwd_scratch_bytes(rows, rows_per_group, groups) + 15) // 16 * 16 + (chunks + 1) * nsg * groups * 8


def gn_apply_grid(rows: int, C: int) -> Tuple[int, int, int, int]:
    """csrc/bwd.hip me_groupnorm_bwd, the apply pass: (ny, bx, by, chunk)."""
    tpr = C // 8
    ny = 1
    while tpr // ny > 256 or tpr % ny:
        ny += 1
    bx = tpr // ny
    by = max(256 // bx, 1)
    chunk = by * 16
    while chunk > by and (rows + chunk - 1) // chunk * ny < 2048:
        chunk //= 2
    return ny, bx, by, max(chunk, by)


def tattn_bwd_path(frames: int, dh: int, heads: int, aligned: bool = True) -> Optional[str]:
    """csrc/bwd.hip me_tattn_bwd: the kernel a call takes, None when it must be refused (the LDS tile of the first version)."""
    hb = {40: 8, 80: 4, 160: 2}[dh]
    if aligned and frames <= 32 and heads % hb == 0:
        return f"tattn_bwd2_kernel<{dh},{hb}>"
    if (4 * frames * dh + 2 * frames * frames) * 4 > 150 * 1024:
        return None
    return "tattn_bwd_kernel"


def tattn_bwd2_lds(frames: int, dh: int) -> int:
    hb = {40: 8, 80: 4, 160: 2}[dh]
    return 4 * hb * frames * dh * 2 + 2 * hb * frames * (frames | 1) * 4


def attn_bwd_path(dh: int) -> str:
    """csrc/attn_bwd.hip me_attn_bwd: keys per block = 64 * NKT, NKT = 2 for dh 40 / 80, 1 for dh 160 (default environment)."""
    return f"attn_bwd_dkv_kernel<{dh},{1 if dh == 160 else 2}>+attn_bwd_dq_kernel"


# ---------------------------------------------------------------------------------------------------------------- the table
CASES = []


def _add(id_, entry, path=None, prod=False, twice=False, bound=None, elementwise=None, **p):
    CASES.append(Case(id=id_, entry=entry, p=p, path=path, prod=prod, twice=twice, bound=bound, elementwise=elementwise))


# ---- gemm_dw (csrc/train.hip:124 dw_geometry, :30 gemm_dw_kernel: 64 x 64 tile, 32-row stages, splits folded in order; :447 me_gemm_dw) ----
DW_EDGE_SHAPES = ((64, 64, 34000), (320, 320, 6000))     # (N, K, sweep limit): one tile -> the 256-split cap binds above M = 32768; 25 tiles -> 41 splits
for _N, _K, _lim in DW_EDGE_SHAPES:
    for _M in dw_edges(_N, _K, _lim):
        _add(f"dw-edge-N{_N}-K{_K}-M{_M}", "gemm_dw", "gemm_dw_kernel", M=_M, N=_N, K=_K)
for _M in (1, 7, 63, 64, 65):                                   # splits == 1, rows below / at / above one stage pair
    _add(f"dw-small-M{_M}", "gemm_dw", "gemm_dw_kernel", M=_M, N=72, K=328)
_add("dw-short-last-split", "gemm_dw", "gemm_dw_kernel", M=513, N=320, K=320)        # 5 splits of 128 rows, the last holds ONE row
_add("dw-swallowed-split", "gemm_dw", "gemm_dw_kernel", M=5000, N=320, K=320)        # 41 splits clamp -> 128-row splits -> 40 splits
for _N, _K in ((8, 8), (72, 8), (8, 72), (320, 328), (328, 320), (72, 72), (328, 328)):     # tails against the 64 x 64 tile
    _add(f"dw-tail-N{_N}-K{_K}", "gemm_dw", "gemm_dw_kernel", M=300, N=_N, K=_K)
_add("dw-alpha", "gemm_dw", "gemm_dw_kernel", M=300, N=320, K=192, alpha=0.37)
_add("dw-f16-lddy-wide", "gemm_dw", "gemm_dw_kernel", M=300, N=320, K=192, dy16=True, dy_pad=24, x_pad=16)
_add("dw-f32-lddy-wide", "gemm_dw", "gemm_dw_kernel", M=300, N=320, K=192, dy_pad=12, x_pad=8, alpha=2.0)
_add("dw-tconv-chunk-lt-frames", "gemm_dw", "gemm_dw_kernel", M=2 * 16 * 12, N=128, K=64, tconv=(16, 12, 8))
_add("dw-tconv-chunk-eq-frames", "gemm_dw", "gemm_dw_kernel", M=2 * 16 * 12, N=128, K=64, tconv=(16, 12, 16))
_add("dw-tconv-chunk-not-dividing", "gemm_dw", "gemm_dw_kernel", M=3 * 14 * 5, N=72, K=64, tconv=(14, 5, 4), alpha=0.5)
_add("dw-tconv-one-frame-chunks", "gemm_dw", "gemm_dw_kernel", M=2 * 6 * 7, N=64, K=64, tconv=(6, 7, 1))           # taps 0 and 2 contribute nothing
_add("dw-twice-bitwise", "gemm_dw", "gemm_dw_kernel", twice=True, M=24 * 1024, N=640, K=640)
_add("dw-prod-L0", "gemm_dw", "gemm_dw_kernel", prod=True, twice=True, M=393216, N=320, K=320)                     # 24 frames of a 128 x 128 latent

# ---- colsum_grad (csrc/train.hip:141: 64 row slices, folded in order) ----
for _M, _N in ((1, 8), (63, 320), (64, 72), (65, 328), (4097, 2560)):
    _add(f"colsum-M{_M}-N{_N}", "colsum_grad", M=_M, N=_N, alpha=1.0 if _M != 65 else -0.25, dy16=_M == 63, dy_pad=0 if _M == 64 else 8)

# ---- gemm_dx (ops.py gemm_dx: me_gemm on transposed, tap-reversed weights; stride 2 -> the zero-stuffed gather, upsampled -> me_grad_acc's pooling) ----
_DX = {
    "dense-odd": dict(M=385, N=320, K=192),
    "dense-n4": dict(M=257, N=4, K=320),
    "geglu-w": dict(M=130, N=2560, K=320),
    "geglu-w-odd": dict(M=67, N=1280, K=640),
    "dense-n4-small": dict(M=7, N=4, K=64),
    "conv-odd": dict(M=3 * 7 * 9, N=128, K=64, conv=(7, 9, 7, 9, 1, 0)),
    "conv-nonsquare": dict(M=2 * 12 * 20, N=64, K=128, conv=(12, 20, 12, 20, 1, 0)),
    "conv-s2-odd-out": dict(M=2 * 5 * 7, N=128, K=64, conv=(10, 14, 5, 7, 2, 0)),
    "conv-s2-nonsquare": dict(M=3 * 4 * 10, N=64, K=64, conv=(8, 20, 4, 10, 2, 0)),
    "conv-ups-odd": dict(M=2 * 10 * 14, N=128, K=64, conv=(5, 7, 10, 14, 1, 1)),
    "conv-ups-nonsquare": dict(M=2 * 8 * 24, N=64, K=64, conv=(4, 12, 8, 24, 1, 1)),
    "tconv-odd": dict(M=3 * 9 * 7, N=128, K=64, tconv=(9, 7, 9)),
    "tconv-chunked": dict(M=2 * 24 * 5, N=64, K=128, tconv=(24, 5, 8)),
}
for _n, _g in _DX.items():
    _add(f"dx-{_n}", "gemm_dx", **_g)
_add("dx-store-nan-prefilled", "gemm_dx", store=True, M=384, N=320, K=192)
_add("dx-store-conv-s2", "gemm_dx", store=True, M=2 * 8 * 8, N=128, K=64, conv=(16, 16, 8, 8, 2, 0))
_add("dx-store-conv-ups", "gemm_dx", store=True, M=2 * 16 * 16, N=128, K=64, conv=(8, 8, 16, 16, 1, 1))
_add("dx-alpha", "gemm_dx", alpha=0.3, M=384, N=320, K=192)
_add("dx-alpha-conv", "gemm_dx", alpha=-1.7, M=2 * 16 * 16, N=128, K=64, conv=(16, 16, 16, 16, 1, 0))
# one production-size launch per UNet level (24 frames of a 128 x 128 latent: 393,216 / 98,304 / 24,576 / 6,144 rows at 320 / 640 / 1280 / 1280 channels)
_add("dx-prod-L0-dense", "gemm_dx", prod=True, M=393216, N=320, K=320)
_add("dx-prod-L1-dense", "gemm_dx", M=98304, N=640, K=640)
_add("dx-prod-L2-tconv", "gemm_dx", M=24 * 32 * 32, N=1280, K=1280, tconv=(24, 1024, 24))
_add("dx-prod-L3-conv", "gemm_dx", M=24 * 16 * 16, N=1280, K=1280, conv=(16, 16, 16, 16, 1, 0))

# ---- attention_bwd (csrc/attn_bwd.hip:61 dK / dV blocks of 64 * NKT keys, :426 dQ blocks of 64 queries; plain segments only) ----
_PC3 = [[0, -1], [0, 1], [1, 2]]                                 # [prev | cur] of three frames
for _n in (1, 63, 64, 65, 127, 128, 129, 257):
    _add(f"attn-nq{_n}-nk{_n}-dh40", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=_n, nk=_n, table=_PC3, n_kv=3)
# nk = 1 with one segment is a softmax over ONE key: P = 1, dS = P (dP - delta) = 0, so dQ and dK are exactly zero under autograd and a relative error has
# nothing to divide by.  `zero` names those outputs; they get the absolute bound of bwd_run.single_key_zero_bound: dP and delta are then the same dh-term
# sum of dO16 * V products taken in two orders, each off by at most (dh - 1) 2^-24 times the sum of the terms' magnitudes.
for _nq, _nk, _dh in ((1, 257, 80), (257, 1, 80), (63, 129, 160), (129, 63, 40), (65, 127, 80), (128, 65, 160)):
    _add(f"attn-nq{_nq}-nk{_nk}-dh{_dh}", "attention_bwd", attn_bwd_path(_dh), dh=_dh, heads=8, nq=_nq, nk=_nk, table=[[0], [1]], n_kv=2,
         **({"zero": ("dq", "dk")} if _nk == 1 else {}))
_add("attn-nseg1-heads1", "attention_bwd", attn_bwd_path(40), dh=40, heads=1, nq=70, nk=70, table=[[0], [1], [2]], n_kv=3)
_add("attn-nseg2-ragged-heads5", "attention_bwd", attn_bwd_path(80), dh=80, heads=5, nq=66, nk=50, table=[[1, -1], [0, 1], [2, -1], [2, 0]], n_kv=3)
_add("attn-nseg3-ragged", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=40, nk=33, table=[[0, 1, 2], [1, -1, -1], [2, 0, -1], [3, 3, 3]], n_kv=4)
_add("attn-unnamed-kv-item", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=64, nk=72, table=[[0, 3], [3, -1], [0, -1]], n_kv=5, unnamed=(1, 2, 4))
_add("attn-kv-named-by-many", "attention_bwd", attn_bwd_path(80), dh=80, heads=8, nq=48, nk=77, table=[[0]] * 9 + [[1]], n_kv=2)
_add("attn-more-kv-than-items", "attention_bwd", attn_bwd_path(160), dh=160, heads=8, nq=32, nk=40, table=[[5, 0], [2, -1]], n_kv=6, unnamed=(1, 3, 4))
_add("attn-fewer-kv-than-items", "attention_bwd", attn_bwd_path(40), dh=40, heads=5, nq=100, nk=77, table=[[0], [0], [0], [0]], n_kv=1)
_add("attn-scale", "attention_bwd", attn_bwd_path(80), dh=80, heads=8, nq=96, nk=96, table=_PC3, n_kv=3, scale=0.05)
_add("attn-fused-qkv-views", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=100, nk=100, table=_PC3, n_kv=3, fused=True)
# the log-sum-exp of each forward form in turn (csrc/attn.hip me_attn: fold from 256 keys, 16 waves from 512 queries, keys resident for 64 < nk <= 80)
_add("attn-lse-classic", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=128, nk=128, table=[[0], [1]], n_kv=2, fwd="attn2_kernel<40,*,classic>")
_add("attn-lse-fold", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=256, nk=257, table=[[0], [1]], n_kv=2, fwd="attn2_kernel<40,2,8,fold>")
_add("attn-lse-fold-16-wave", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=512, nk=256, table=[[0, 1], [1, -1]], n_kv=2, fwd="attn2_kernel<40,2,16,fold>")
_add("attn-lse-kvres", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=520, nk=77, table=[[0], [0], [1]], n_kv=2, fwd="attn2_kernel<40,*,8,kvres>")
_add("attn-peaked-fallback", "attention_bwd", attn_bwd_path(40), dh=40, heads=8, nq=96, nk=640, table=[[0], [1]], n_kv=2, peaked=15.0, fwd="attn2_kernel<40,*,fold>")

# ---- temporal_attention_bwd (csrc/bwd.hip me_tattn_bwd: lane-parallel kernel for frames <= 32, aligned rows, heads % (8 / 4 / 2) == 0; else the first version) ----
TATTN_FRAMES = (1, 2, 7, 8, 25, 31, 32, 33, 40, 48, 64)
for _F in TATTN_FRAMES:
    for _dh in (40, 80, 160):
        _path = tattn_bwd_path(_F, _dh, 8)
        if _path is None:
            continue                                             # frames = 64, dh = 160: refused (TATTN_REFUSED below)
        _add(f"tattn-F{_F}-dh{_dh}", "temporal_attention_bwd", _path, frames=_F, dh=_dh, heads=8, npix=3, batch=2 if _F < 40 else 1)
TATTN_REFUSED = dict(frames=64, dh=160, heads=8, npix=1, batch=1)
for _dh, _heads in ((40, 5), (40, 12), (40, 16), (80, 5), (80, 2), (80, 12), (160, 1), (160, 5), (160, 4)):      # heads missing / meeting the 8 / 4 / 2 rule
    _add(f"tattn-heads{_heads}-dh{_dh}", "temporal_attention_bwd", tattn_bwd_path(24, _dh, _heads), frames=24, dh=_dh, heads=_heads, npix=2, batch=1)
for _np in (1, 63, 64, 65, 257):
    _add(f"tattn-npix{_np}", "temporal_attention_bwd", tattn_bwd_path(8, 40, 8), frames=8, dh=40, heads=8, npix=_np, batch=2)
_add("tattn-npix65-first-version", "temporal_attention_bwd", tattn_bwd_path(33, 80, 8), frames=33, dh=80, heads=8, npix=65, batch=1)
_add("tattn-ld-wide-fused-qkv", "temporal_attention_bwd", tattn_bwd_path(24, 80, 8), frames=24, dh=80, heads=8, npix=5, batch=2, fused=True, do_pad=8)
_add("tattn-ld-wide-first-version", "temporal_attention_bwd", tattn_bwd_path(48, 40, 8), frames=48, dh=40, heads=8, npix=3, batch=1, fused=True, do_pad=4)
_add("tattn-rows-off-16-bytes", "temporal_attention_bwd", tattn_bwd_path(24, 40, 8, aligned=False), frames=24, dh=40, heads=8, npix=3, batch=1, q_off=4)
_add("tattn-scale", "temporal_attention_bwd", tattn_bwd_path(16, 160, 8), frames=16, dh=160, heads=8, npix=2, batch=1, scale=0.2)

# ---- groupnorm_bwd (csrc/bwd.hip gn_bwd_chunks: chunk_rows >= 8, <= 512 chunks, one chunk beyond 1024 statistic groups; the apply pass's ny / chunk grid) ----
for _C in (320, 640, 960, 1280, 1920, 2560):
    _add(f"gn-C{_C}", "groupnorm_bwd", twice=_C in (320, 2560), C=_C, rpg=50 if _C > 1280 else 97, nsg=3, silu=_C % 640 == 0)
for _rpg in (1, 7, 8, 9):
    _add(f"gn-rpg{_rpg}", "groupnorm_bwd", C=320, rpg=_rpg, nsg=3, silu=_rpg % 2 == 1)
# nsg = 2 -> 512 chunks: rows_per_group 4096 -> chunk_rows 8 (full), 4095 (short last chunk), 4097 -> chunk_rows 9, 456 chunks (last one holds 2 rows)
for _rpg in (4095, 4096, 4097, 6143, 6145):
    _add(f"gn-chunk-edge-rpg{_rpg}", "groupnorm_bwd", C=320, rpg=_rpg, nsg=2, silu=True)
_add("gn-nsg1", "groupnorm_bwd", C=640, rpg=1030, nsg=1, silu=False)                # 512 chunks of 3 -> floored to 8 rows: 129 chunks
_add("gn-nsg1025", "groupnorm_bwd", C=320, rpg=9, nsg=1025, silu=True)              # 1024 / nsg = 0 -> one chunk per statistic group
_add("gn-nsg1025-rpg1", "groupnorm_bwd", C=640, rpg=1, nsg=1025, silu=False)
_add("gn-large-mean-C320", "groupnorm_bwd", twice=True, C=320, rpg=2048, nsg=2, silu=True, mean=100.0, spread=1.0)
_add("gn-large-mean-C1280", "groupnorm_bwd", C=1280, rpg=64, nsg=8, silu=False, mean=100.0, spread=1.0)

# ---- layernorm_bwd / layernorm_bwd_params (csrc/bwd.hip:36 one wave per row, 4 rows per block; csrc/train.hip ln_params_blocks: >= 64 rows per block, <= 512 blocks) ----
for _rows in (1, 3, 4, 5):
    for _C in (320, 640, 1280):
        _add(f"ln-rows{_rows}-C{_C}", "layernorm_bwd", rows=_rows, C=_C)
        _add(f"lnp-rows{_rows}-C{_C}", "layernorm_bwd_params", rows=_rows, C=_C)
_add("ln-rows70001-C320", "layernorm_bwd", rows=70001, C=320)
_add("lnp-rows70001-C320", "layernorm_bwd_params", rows=70001, C=320)
_add("ln-large-mean", "layernorm_bwd", rows=130, C=640, mean=100.0, spread=1.0)
_add("lnp-large-mean", "layernorm_bwd_params", rows=130, C=640, mean=100.0, spread=1.0)
_add("ln-strided-x-dy-dx", "layernorm_bwd", rows=77, C=320, x_pad=8, dy_pad=12, dx_pad=20)
_add("lnp-strided-x-dy", "layernorm_bwd_params", rows=257, C=1280, x_pad=8, dy_pad=12)
_add("lnp-dgamma-only", "layernorm_bwd_params", rows=65, C=320, only="dgamma")
_add("lnp-dbeta-only", "layernorm_bwd_params", rows=65, C=320, only="dbeta")

# ---- geglu_bwd (csrc/bwd.hip:21).  Overflow contract (ops.geglu_bwd returns fp16 and says no more): the fp32 product is converted with round-to-nearest, so a
#      product beyond fp16's range becomes +-inf of the right sign -- it is neither clamped nor turned into NaN; finite products next to it are unaffected. ----
for _M, _N in ((1, 32), (3, 64), (255, 64), (257, 2560), (300, 640)):
    _add(f"geglu-M{_M}-N{_N}", "geglu_bwd", M=_M, N=_N)
_add("geglu-far-tails", "geglu_bwd", M=64, N=64, amp=12.0)
_add("geglu-strided-dy", "geglu_bwd", M=130, N=640, dy_pad=8)
# geglu-fp16-overflow holds finite gradients up to 6.45e4 next to a mean of ~1: one fp16 ulp there (32) is 30 times the mean, so max / mean <= 2e-2 cannot be
# met by ANY fp16 output.  Its finite elements get elementwise="geglu-f16-range" instead: 2^-10 |d pre| (half an fp16 ulp, 2^-11 relative, doubled) plus
# 2^-20 |dy| (1 + |value|) for erff / __expf evaluated in fp32 (a few 2^-24 of Phi(gate) + gate phi(gate) <= 1.13, times the factor dy * value).  rel-L2 over
# the finite elements stays the entry point's 2e-3; the elements the reference puts beyond 65520 must be +-inf of the right sign.  The fp32 emulation (which
# keeps fp32, so only the second term is exercised) stays inside the same limit on this CPU: tests/test_bwd_sweep_cpu.py.
_add("geglu-fp16-overflow", "geglu_bwd", M=16, N=64, overflow=True, elementwise="geglu-f16-range")

# ---- softmax_bwd_rows (csrc/bwd.hip: one wave per row, 8 columns per lane and pass), relu_bwd, grad_acc, casts ----
# me_softmax_bwd_rows had no test and so no stated bound.  rel-L2: the per-kernel 2e-3 of fp16 storage.  Per element, elementwise="f16-out" in place of
# max / mean: dS = P (dP - delta) scale of a peaked softmax row spans many binades (max |dS| / mean |dS| reaches hundreds at 4096 columns), and the error of an
# fp16 output is relative to EACH element, so max-error / mean-magnitude would measure how peaked the row is.  The limit: 2^-10 |dS| (half an fp16 ulp, 2^-11,
# doubled) + 2^-20 (1 + max |dS|) for the fp32 evaluation of P (dP - delta) on exact fp16 inputs (a few 2^-24 of |P| (|dP| + |delta|); it also covers
# results in fp16's subnormal range, whose spacing is 2^-24).
for _r, _c in ((1, 8), (3, 72), (5, 512), (130, 520), (9, 4096)):
    _add(f"smbwd-{_r}x{_c}", "softmax_bwd_rows", rows=_r, cols=_c, pad=0 if _c == 512 else 8, scale=0.158 if _c == 72 else 1.0, elementwise="f16-out")
for _r, _c in ((1, 1), (3, 255), (257, 320), (1000, 7)):
    _add(f"relu-{_r}x{_c}", "relu_bwd", rows=_r, cols=_c, pad=0 if _r == 1 else 3)
_add("gacc-f32-strided", "grad_acc", rows=301, cols=68, pad=8, alpha=0.5)
_add("gacc-f16-strided", "grad_acc", rows=301, cols=68, pad=8, alpha=-2.0, f16=True)
_add("gacc-one-row", "grad_acc", rows=1, cols=4, pad=0, alpha=1.0)
_add("gacc-store-nan-prefilled", "grad_acc", rows=65, cols=64, pad=4, alpha=0.25, store=True)
_add("gacc-pool-odd", "grad_acc", rows=3 * 5 * 7, cols=64, pad=4, alpha=1.0, f16=True, pool=(5, 7))
_add("gacc-pool-1x1", "grad_acc", rows=4, cols=8, pad=0, alpha=1.0, pool=(1, 1))
_add("gacc-pool-store-f32", "grad_acc", rows=2 * 3 * 9, cols=320, pad=8, alpha=0.5, pool=(3, 9), store=True)
_add("gacc-flat", "grad_acc", rows=1, cols=77 * 768, pad=0, alpha=2.0, flat=True)
for _r, _c, _pc in ((1, 4, 4), (50, 20, 24), (257, 4, 8), (33, 320, 320)):
    _add(f"castrows-{_r}x{_c}-pad{_pc}", "cast_rows_f16", rows=_r, cols=_c, pad_cols=_pc, off=4 if _c == 20 else 0)
for _n in (1, 255, 256, 257, 100_003):
    _add(f"cast-n{_n}", "cast_f16", n=_n)
_add("mse-seed-full", "mse_seed", nb=1, C=4, f=3, h=5, w=7, full=True)
_add("mse-seed-plain-nb2", "mse_seed", nb=2, C=4, f=2, h=3, w=3, full=False)

# ---- adamw (csrc/train.hip:307; grid-stride over 256-thread blocks, <= 8192 blocks) ----
for _n in (1, 255, 256, 257, 3_000_001):
    _add(f"adamw-n{_n}-step1", "adamw", n=_n, step=1, wd=1e-2, clip=None)
_add("adamw-step10000", "adamw", n=1000, step=10_000, wd=1e-2, clip=None)
_add("adamw-tiny-g-zero-v", "adamw", n=1000, step=1, wd=0.0, clip=None, tiny=True)      # v == 0, |g| ~ 1e-9: the update is lr g / (|g| + eps), eps decides
_add("adamw-clip-below-1", "adamw", n=5000, step=3, wd=1e-2, clip="active")               # norm above max_grad_norm: the factor is < 1
_add("adamw-clip-above-1", "adamw", n=5000, step=3, wd=0.0, clip="idle")                  # norm below max_grad_norm: min(1, .) keeps the gradient
_add("adamw-no-decay-step2", "adamw", n=257, step=2, wd=0.0, clip=None, moments=True)
_add("adamw-gnorm-inf", "adamw", n=1000, step=1, wd=1e-2, clip="inf")                      # me_adamw: a no-op, p, m, v bitwise unchanged
_add("adamw-gnorm-nan", "adamw", n=1000, step=1, wd=1e-2, clip="nan")

# ---- sumsq_absmax (csrc/train.hip: 1024 blocks x 256 threads over ceil(n / 1024) elements each; max |x| propagates NaN -- include/motioned.h) ----
for _n in (1, 255, 256, 257, 1024, 1025, 262_144, 262_145, 3_000_001):
    _add(f"sumsq-n{_n}", "sumsq_absmax", n=_n)
SUMSQ_N = 300_007                                                # 293 elements per block; the last block holds 268: its threads' second pass is a 12-element tail
for _kind in ("nan", "+inf", "-inf"):
    for _pos in ("first", "last", "tail", "alone"):
        _add(f"sumsq-{_kind}-{_pos}", "sumsq_absmax", n=1 if _pos == "alone" else SUMSQ_N, special=_kind, pos=_pos)
_add("sumsq-nan-and-inf", "sumsq_absmax", n=SUMSQ_N, special="nan", pos="first", also_inf=True)

BY_ID = {c.id: c for c in CASES}
ENTRIES = sorted({c.entry for c in CASES})


def case_counts() -> Dict[str, int]:
    out: Dict[str, int] = {}
    for c in CASES:
        out[c.entry] = out.get(c.entry, 0) + 1
    return out


def elementwise_limit(case, w):
    """The per-element error limit |got - want| <= limit of a case that names one (`elementwise=`; derivations next to the entries), from the fp64 result w."""
    p = case.p
    w = w.double().abs()
    if case.elementwise == "f16-out":
        return 2.0 ** -10 * w + 2.0 ** -20 * (1.0 + float(w.max()))
    if case.elementwise == "geglu-f16-range":
        t = build(case)
        M, N = p["M"], p["N"]
        dy = t["dy"][:, :N // 2].double().abs().reshape(M, N // 32, 1, 16)
        val = t["pre"].double().abs().reshape(M, N // 32, 2, 16)[:, :, 0:1]
        return 2.0 ** -10 * w + (2.0 ** -20 * dy * (1.0 + val)).expand(M, N // 32, 2, 16).reshape(M, N)
    raise KeyError(case.elementwise)


# ---------------------------------------------------------------------------------------------------------------- seeded input builders (CPU tensors)
def _gen(case):
    return torch.Generator().manual_seed(seed_of(case.id))


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _wide(t, pad, off=0, fill=0.0):
    """t embedded at column `off` of a tensor `pad` columns wider: (the wide tensor, the view)."""
    big = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    big[:, off:off + t.shape[1]] = t
    return big


def build(case) -> dict:
    """The CPU input tensors of a case, fp16 / fp32 as the HIP entry point takes them.  `*_base` are the full allocations, views are cut by the runner."""
    p, g, e = case.p, _gen(case), case.entry
    if e == "gemm_dw":
        M, N, K = p["M"], p["N"], p["K"]
        taps = 3 if p.get("tconv") else 1
        x = _wide(_randn(g, M, K).half(), p.get("x_pad", 0))
        dy = _randn(g, M, N)
        dy = _wide(dy.half() if p.get("dy16") else dy, p.get("dy_pad", 0), fill=7.0)     # the padding columns hold a value that must not be read
        return dict(x=x, dy=dy, base=_randn(g, N, taps, K, scale=0.5))
    if e == "colsum_grad":
        dy = _randn(g, p["M"], p["N"])
        return dict(dy=_wide(dy.half() if p.get("dy16") else dy, p.get("dy_pad", 0), fill=7.0), base=_randn(g, p["N"], scale=0.5))
    if e == "gemm_dx":
        M, N, K = p["M"], p["N"], p["K"]
        conv, tconv = p.get("conv"), p.get("tconv")
        taps = 9 if conv else (3 if tconv else 1)
        xr = (M // (conv[2] * conv[3])) * conv[0] * conv[1] if conv else M
        w = _randn(g, N, taps, K, scale=(taps * K) ** -0.5).half()
        dy = _randn(g, M, N)
        base = torch.full((xr, K + 8), float("nan")) if p.get("store") else _randn(g, xr, K + 8, scale=0.5)
        return dict(w=w, dy=dy, base=base, xr=xr, taps=taps)
    if e == "attention_bwd":
        dh, heads, nq, nk, n_kv = p["dh"], p["heads"], p["nq"], p["nk"], p["n_kv"]
        C, n_items = heads * dh, len(p["table"])
        q, k = _randn(g, n_items * nq, C, scale=0.7), _randn(g, n_kv * nk, C, scale=0.7)
        v, dout = _randn(g, n_kv * nk, C), _randn(g, n_items * nq, C)
        if p.get("peaked"):      # after tests/test_kernels_gpu.py test_attention_fixed_offset_overflow_...: 32 keys of the last tiles sit p["peaked"] nats above the
            # typical logit.  15 nats = 21.6 binades: past the 2^16 a fixed-offset P may reach, so the forward's blocks fall back to the running maximum.  The
            # mass is shared by 32 keys with different values, which keeps dS = P (dP - sum P dP) well conditioned: ONE hot key would make it the difference of
            # two nearly equal numbers (the fp32 emulation itself is then 9e-2 off the fp64 reference on dK)
            q, k = q * (0.5 / 0.7), k * (0.5 / 0.7)
            scale = dh ** -0.5
            for it in range(n_items):
                for h in range(heads):
                    qs = q[it * nq:(it + 1) * nq, h * dh:(h + 1) * dh]
                    d = qs.mean(0)
                    d = d / d.norm()
                    qs += d * 3.0
                    k[p["table"][it][0] * nk + nk - 102:p["table"][it][0] * nk + nk - 70, h * dh:(h + 1) * dh] += d * (p["peaked"] / (3.0 * scale))
        width = lambda: 3 * C if p.get("fused") else C    # noqa: E731
        bases = [_randn(g, r, width(), scale=0.5) for r in (n_items * nq, n_kv * nk, n_kv * nk)]
        nseg = max(len(r) for r in p["table"])
        tab = torch.tensor([list(r) + [-1] * (nseg - len(r)) for r in p["table"]], dtype=torch.int32)
        return dict(q=q.half(), k=k.half(), v=v.half(), dout=dout, dq=bases[0], dk=bases[1], dv=bases[2], seg_item=tab, seg_mode=torch.zeros_like(tab))
    if e == "temporal_attention_bwd":
        C, rows = p["heads"] * p["dh"], p["batch"] * p["frames"] * p["npix"]
        return dict(qkv=_randn(g, rows, 3 * C, scale=0.7).half(), dout=_randn(g, rows, C))
    if e == "groupnorm_bwd":
        C, rows = p["C"], p["rpg"] * p["nsg"]
        x = _randn(g, rows, C) * p.get("spread", 1.5) + p.get("mean", 0.5)
        return dict(x=x.half(), gamma=(1 + 0.2 * _randn(g, C)).half(), beta=(0.2 * _randn(g, C)).half(), dy=_randn(g, rows, C))
    if e in ("layernorm_bwd", "layernorm_bwd_params"):
        rows, C = p["rows"], p["C"]
        x = (_randn(g, rows, C) * p.get("spread", 2.0) + p.get("mean", 0.3)).half()
        d = dict(x=_wide(x, p.get("x_pad", 0)), dy=_wide(_randn(g, rows, C), p.get("dy_pad", 0), fill=7.0), gamma=(1 + 0.2 * _randn(g, C)).half())
        d.update(dgamma=_randn(g, C, scale=0.5), dbeta=_randn(g, C, scale=0.5))
        return d
    if e == "geglu_bwd":
        M, N = p["M"], p["N"]
        pre, dy = _randn(g, M, N, scale=1.5), _randn(g, M, N // 2)
        if p.get("amp"):
            pre = (torch.rand(M, N, generator=g) * 2 - 1) * p["amp"]          # |pre| up to 12: Phi(-12) ~ 1e-33, the far GELU tails
            pre[0, 16:32] = torch.linspace(-p["amp"], p["amp"], 16)
        if p.get("overflow"):                                                 # dy * gelu(gate) and dy * val * gelu'(gate) beyond 65504 in chosen places
            pre = pre.clamp(-4, 4)
            pre[0, 16] = 8.0
            dy[0, 0] = 3.0e4          # d value = 3e4 * gelu(8) = 2.4e5 -> +inf
            pre[1, 1], pre[1, 17] = 300.0, 5.0
            dy[1, 1] = -1.0e3         # d gate = -1e3 * 300 * gelu'(5) = -3e5 -> -inf;  d value = -1e3 * gelu(5) = -5e3, finite
            pre[2, 2], pre[2, 18] = 1.0, 2.0
            dy[2, 2] = 3.3e4          # 3.3e4 * gelu(2) = 6.45e4: just inside the range, stays finite
        return dict(pre=pre.half(), dy=_wide(dy, p.get("dy_pad", 0), fill=7.0))
    if e == "softmax_bwd_rows":
        P = torch.softmax(_randn(g, p["rows"], p["cols"], scale=2.0), dim=-1).half()
        return dict(P=_wide(P, p["pad"]), dP=_wide(_randn(g, p["rows"], p["cols"]).half(), p["pad"]))
    if e == "relu_bwd":
        return dict(dy=_wide(_randn(g, p["rows"], p["cols"]), p["pad"]), out=_wide(_randn(g, p["rows"], p["cols"]).half(), p["pad"]))
    if e == "grad_acc":
        rows, cols = p["rows"], p["cols"]
        srows = 4 * rows if p.get("pool") else rows + (0 if p.get("flat") else 5)
        src = _randn(g, srows, cols)
        src = _wide(src.half() if p.get("f16") else src, 0 if p.get("flat") else 8, fill=7.0)
        base = torch.full((rows, cols + 2 * p["pad"]), float("nan")) if p.get("store") else _randn(g, rows, cols + 2 * p["pad"], scale=0.5)
        return dict(src=src, base=base)
    if e == "cast_rows_f16":
        return dict(src=_randn(g, p["rows"], p["cols"] + 2 * p["off"] + 4, scale=10.0))
    if e == "cast_f16":
        return dict(src=_randn(g, p["n"], scale=10.0))
    if e == "mse_seed":
        nb, C, f, h, w = p["nb"], p["C"], p["f"], p["h"], p["w"]
        rows = nb * f * h * w
        return dict(eu=_randn(g, rows, 8).half(), ec=_randn(g, rows, 8).half(), x=_randn(g, nb, C, f, h, w), target=_randn(g, nb, C, f, h, w))
    if e == "adamw":
        n = p["n"]
        d = dict(p=_randn(g, n), g=_randn(g, n) * (1e-9 if p.get("tiny") else 3.0))
        d["m"], d["v"] = (_randn(g, n, scale=0.1), _randn(g, n, scale=0.1).abs()) if p.get("moments") or p["step"] > 1 else (torch.zeros(n), torch.zeros(n))
        if p["clip"] == "idle":
            d["g"] = d["g"] * (0.5 / float(d["g"].norm()))                   # norm 0.5 < max_grad_norm 1
        return d
    if e == "sumsq_absmax":
        n = p["n"]
        x = _randn(g, n, scale=3.0)
        if n > 2:
            x[n // 2] = -40.0                                                 # the exact maximum, negative
        if p.get("special"):
            val = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[p["special"]]
            per = (n + 1023) // 1024
            idx = {"first": 0, "last": n - 1, "alone": 0, "tail": min(((n - 1) // per) * per + 260, n - 2)}[p["pos"]]
            x[idx] = val
            if p.get("also_inf"):
                x[n - 2] = float("inf")
        return dict(x=x)
    raise KeyError(e)
