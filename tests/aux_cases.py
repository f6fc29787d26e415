"""TEST INFRASTRUCTURE: the case table of the third sweep (tests/test_aux_sweep_cpu.py, tests/test_aux_sweep_gpu.py): every entry point the backward sweep
(tests/bwd_cases.py) and the forward sweep (tests/fwd_cases.py) left out -- me_conv_dw, me_groupnorm_bwd_params, me_refresh_weights / me_refresh_ups4,
me_conv_small, the flat and row-wise kernels of csrc/eltwise.hip and csrc/clip.hip, the step scalars and layout converters, me_attn_causal.

Same method as the other two tables: the launch code is restated in Python (below; the file and line stand next to each family), a case sits on both sides
of every point where the launch code changes, and tests/test_aux_sweep_cpu.py checks the restatement against the library's host functions and shows that
the fp32 emulation reaches the entry point's bound on every case while a set of deliberately wrong emulations does not.  Case, seed_of and the
bound= / elementwise= / zero= rules are tests/bwd_cases.py's.  csrc/image.hip stays out: tests/test_clip_io_cpu.py / test_clip_io_gpu.py already restate
its modes, sizes and awkward views.

What the restatements find UNREACHABLE:
  cw_geometry, the 256 MiB clamp: it decides only where ceil(1024 / tiles) > floor(2^28 / (36 N K)).  With N K <= 4096 tiles that needs
      ceil(1024 / tiles) > floor(1820.4 / tiles), which holds for 911 <= tiles <= 1023 alone (two splits wanted, one allowed; from 1024 tiles on one split is
      wanted and a scratch below one split is refused by the host).  The brute-force scan of tests/test_aux_sweep_cpu.py confirms it over every multiple-of-64
      shape; N = 1920, K = 2048 (960 tiles) with M >= 129 is such a shape: case cdw-scratch-clamp (prod: 141 MB of weight gradient).
  cw_geometry, "cap256" deciding at 320 x 320: 25 tiles want 41 splits, below the cap at any M.
  gn_params_blocks: beyond one block rows_per_block lies in 33 .. 64 until the 512-block cap binds (rows > 32768) and grows from there; a block of fewer than 33 rows
      next to others does not occur.
  grid_for(cap 4096) of the conv_dw fold wraps from N * 9 * K > 4096 * 1024 on: N = K = 704 is the smallest square multiple of 64 (cdw-fold-wraps).
No case uses bound=."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

import bwd_cases as bc
from bwd_cases import MAX_REL, REL_L2, Case, seed_of

# ---------------------------------------------------------------------------------------------------------------- bounds (rel-L2, max-abs / mean-abs)
EXACT = (0.0, 0.0)
BOUNDS: Dict[str, Tuple[float, float]] = {
    "conv_dw": bc.BOUNDS["gemm_dw"],                               # tests/test_tune_conv_gpu.py test_conv_dw_matches_the_fp64_reference
    "gn_params.dgamma": bc.BOUNDS["layernorm_bwd_params.dgamma"],  # ... test_groupnorm_bwd_params_matches_fp64_autograd
    "gn_params.dbeta": bc.BOUNDS["layernorm_bwd_params.dbeta"],
    "refresh": EXACT,                                              # bitwise weights.Packed.ln_fold / fold_ups; colsum / cvec: aux_run.refresh_vector_bound
    "conv_small": (REL_L2, MAX_REL),                               # tests/test_kernels_gpu.py check()
    "axpy_rows": (REL_L2, MAX_REL),
    "silu": (REL_L2, MAX_REL),
    "quick_gelu": (REL_L2, MAX_REL),                               # tests/test_clip_gpu.py check()
    "attention_causal": (REL_L2, MAX_REL),
    "timestep_embed": (2e-3, MAX_REL),                             # test_elementwise_family: rel=2e-3
    "cfg_ddim": (1e-5, 1e-4),                                      # test_elementwise_family: rel=1e-5, mx=1e-4
    "gaussian_sample": (REL_L2, MAX_REL),                          # tests/test_guard_gpu.py check()
    "nchw_to_rows": (REL_L2, MAX_REL),                             # (one fp16 rounding)
    "rows_to_nchw": EXACT,                                         # fp16 -> fp32 is exact
    "copy_rows": EXACT, "copy_blocks": EXACT, "relu": EXACT, "embed_rows": EXACT,
}


# ---------------------------------------------------------------------------------------------------------------- launch geometry, restated
CW_CAP = 256 << 20


def cw_geometry(M: int, N: int, K: int) -> Tuple[int, int, str]:
    """csrc/tune.hip:153 cw_geometry -> (splits, rows_per_split, the clamp that decided the split count)."""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    s, why = (1024 + tiles - 1) // tiles, "tiles"              # ~1024 blocks
    smax = (M + 4 * 32 - 1) // (4 * 32)                         # at least four 32-row stages per split
    scap = CW_CAP // (N * 9 * K * 4)                            # the partials stay inside 256 MiB
    if s > smax:
        s, why = smax, "stages"
    if s > scap:
        s, why = scap, "scratch"
    if s > 256:
        s, why = 256, "cap256"
    if s < 1:
        s = 1
    rps = (M + s - 1) // s
    rps = (rps + 31) // 32 * 32
    return (M + rps - 1) // rps, rps, why


def cw_work_bytes(M: int, N: int, K: int) -> int:
    return cw_geometry(M, N, K)[0] * N * 9 * K * 4 if min(M, N, K) > 0 else 0


def cw_edges(N: int, K: int, m_max: int, interior: int = 1):
    """bwd_cases.dw_edges on cw_geometry: the M on both sides of every change of the deciding clamp and of splits 1 -> 2, plus the first, the last and
    `interior` evenly spaced ones of the points inside each regime where splits or rows_per_split changes (a SUB-SAMPLE, as there)."""
    picks, prev, changes = set(), None, {}
    for M in range(1, m_max + 1):
        cur = cw_geometry(M, N, K)
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


def gn_params_blocks(rows: int) -> Tuple[int, int]:
    """csrc/tune.hip:218 gn_params_blocks and me_groupnorm_bwd_params -> (blocks launched, rows_per_block); blocks past ceil(rows / rows_per_block) hold no row."""
    b = max(1, min(512, (rows + 63) // 64))
    return b, (rows + b - 1) // b


def gn_params_work_bytes(rows: int, rpg: int, C: int, groups: int) -> int:
    return (bc.gn_fwd_scratch_bytes(rows, rpg, groups) + 15) // 16 * 16 + gn_params_blocks(rows)[0] * 2 * C * 4


def grid_for(n: int, cap: int) -> int:
    """csrc/eltwise.hip:257, csrc/clip.hip:185 (cap 16384), csrc/tune.hip:248 (cap 4096: the conv_dw fold; 8192: refresh_ups4): 256-thread blocks."""
    return max(1, min(cap, (n + 255) // 256))


FLAT_CAP = 16384
FLAT_EDGE = FLAT_CAP * 256            # work items (vectors) one pass of the grid-stride loop covers


def conv_small_target(Cin: int, Cout: int) -> str:
    """csrc/eltwise.hip:284 me_conv_small: the 64-pixel tile kernel for 64 <= Cout <= 480, Cout % 32 == 0; else the direct kernel (80-channel slices)."""
    tile = 64 <= Cout <= 480 and Cout % 32 == 0
    return f"conv_small_tile_kernel<{Cin}>" if tile else f"conv_small_kernel<{Cin}>"


def conv_small_geometry(Cin: int, Cout: int, npix: int) -> Tuple[int, int, int]:
    """(pixels per block, pixel blocks, channel slices) of the launch."""
    if conv_small_target(Cin, Cout).startswith("conv_small_tile"):
        return 64, (npix + 63) // 64, 1
    co = 80 if Cout > 80 else Cout
    return 256, (npix + 255) // 256, (Cout + co - 1) // co


def attn_causal_geometry(nq: int):
    """csrc/clip.hip:59 attn_causal_kernel: per 64-query block (nkeys, nkeys_pad, [nt of each of its four waves; 0: the wave returns after the barrier])."""
    out = []
    for qb0 in range(0, nq, 64):
        nkeys = min(nq, qb0 + 64)
        nts = [min((qb0 + w * 16) // 16 + 1, (nkeys + 15) >> 4) if qb0 + w * 16 < nq else 0 for w in range(4)]
        out.append((nkeys, (nkeys + 31) & ~31, nts))
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
CASES = []


def _add(id_, entry, path=None, prod=False, twice=False, bound=None, elementwise=None, **p):
    CASES.append(Case(id=id_, entry=entry, p=p, path=path, prod=prod, twice=twice, bound=bound, elementwise=elementwise))


# ---- conv_dw (csrc/tune.hip:153 cw_geometry, :40 conv_dw_kernel: 64 x 64 x 9 tile, 32-row stages; :138 the fold, grid capped at 4096; :278 me_conv_dw) ----
def conv_out(Hin, Win, stride, ups):
    return ((Hin << ups) - 1) // stride + 1, ((Win << ups) - 1) // stride + 1


def _cdw(id_, n_img, Hin, Win, N, K, stride=1, ups=0, **kw):
    Hout, Wout = conv_out(Hin, Win, stride, ups)
    M = n_img * Hout * Wout
    kw.setdefault("twice", cw_geometry(M, N, K)[0] > 1)
    _add(id_, "conv_dw", "conv_dw_kernel<f16>" if kw.get("dy16") else "conv_dw_kernel<f32>", n_img=n_img, Hin=Hin, Win=Win, N=N, K=K, stride=stride, ups=ups, M=M, **kw)


def image_for(M: int) -> Tuple[int, int, int]:
    """(n_img, H, W) with n_img * H * W == M, the largest of the small images 5x7, 2x2, 1x3, 1x1 that divides M: M moves in fine steps."""
    for H, W in ((5, 7), (2, 2), (1, 3), (1, 1)):
        if M % (H * W) == 0:
            return M // (H * W), H, W


# (N, K, sweep limit): one tile -> the 256-split cap binds above M = 32640; 2 and 3 tiles alike; 25 tiles -> 41 splits above M = 5248
CW_EDGE_SHAPES = ((64, 64, 33000), (40, 72, 33000), (8, 8, 33000), (56, 136, 33000), (320, 320, 6000))
for _N, _K, _lim in CW_EDGE_SHAPES:
    for _M in cw_edges(_N, _K, _lim):
        _cdw(f"cdw-edge-N{_N}-K{_K}-M{_M}", *image_for(_M), _N, _K)
for _n in (1, 2, 31, 32, 33, 63, 64, 65, 95, 97):                # M below one 32-row stage (the 1 x 1-pixel level), M = 32 k +- 1: n images of 1 x 1
    _cdw(f"cdw-1x1-M{_n}", _n, 1, 1, 40, 72)
_cdw("cdw-short-last-split", 513, 1, 1, 320, 320)                # 5 splits of 128 rows, the last holds ONE row
_cdw("cdw-swallowed-split", 1250, 2, 2, 320, 320)                # M = 5000: the 41-split clamp -> 128-row splits cover it in 40
for _s, _u, _H, _W in ((1, 0, 5, 7), (1, 0, 4, 6), (2, 0, 5, 7), (2, 0, 4, 6), (2, 0, 7, 4), (1, 1, 3, 5), (1, 1, 2, 2), (1, 0, 1, 9), (1, 0, 9, 1), (2, 0, 1, 9), (2, 0, 9, 1),
                       (1, 1, 1, 4), (1, 1, 4, 1)):              # stride 1 / 2 at odd and even Hin, Win; ups 1; Hin = 1 or Win = 1
    _cdw(f"cdw-s{_s}-u{_u}-{_H}x{_W}", 3, _H, _W, 40, 72, stride=_s, ups=_u)
_cdw("cdw-split-inside-an-image-row", 4, 5, 7, 40, 72)          # M = 140: 2 splits of 96 rows; row 96 is pixel (3, 5) of image 2
_cdw("cdw-split-inside-a-row-s2", 12, 9, 13, 56, 136, stride=2)  # 5 x 7 outputs of a 9 x 13 input, M = 420: 4 splits of 128 rows
_cdw("cdw-split-inside-a-row-ups", 4, 3, 5, 56, 136, ups=1)      # 6 x 10 outputs, M = 240: 2 splits of 128 rows
_cdw("cdw-f16-dy", 4, 5, 7, 40, 72, dy16=True)
_cdw("cdw-f16-dy-wide", 4, 5, 7, 64, 64, dy16=True, dy_pad=24, x_pad=16, alpha=0.37)
_cdw("cdw-f32-dy-wide", 4, 5, 7, 64, 64, dy_pad=12, x_pad=8, alpha=2.0)
_cdw("cdw-alpha", 5, 5, 7, 320, 320, alpha=-0.5)
_cdw("cdw-fold-wraps", 3, 1, 3, 704, 704, alpha=0.25)            # N * 9 * K = 4,460,544 > 4096 * 1024: 4357 fold blocks wanted, 4096 launched
_cdw("cdw-scratch-clamp", 4, 5, 7, 1920, 2048, prod=True)        # 960 tiles, M = 140: two splits wanted and allowed by the stages, ONE by the 256 MiB scratch
CONV_DW_REFUSED = (                                             # (label, overrides of a valid 2 x 5 x 7, N = 40, K = 72 call, needle of the message)
    ("N 9 K fp32 beyond 256 MiB", dict(N=2816, K=2656, lddy=2816, ldx=2656), "256 MiB"), ("pad0", dict(pad0=1), "pad0"), ("ups 2", dict(ups=2, Hout=10, Wout=14, M=280), "ups must be"),
    ("ups 3", dict(ups=3), "ups must be"), ("stride 2 with ups", dict(stride=2, ups=1), "stride 2 together"), ("M not whole images", dict(M=69), "bad conv geometry"),
    ("Hout wrong", dict(Hout=4), "bad conv geometry"), ("N % 8", dict(N=44), "multiples of 8"), ("lddy < N", dict(lddy=32), "multiples of 8"), ("ldx % 8", dict(ldx=76), "multiples of 8"),
    ("stride 3", dict(stride=3), "stride must be"), ("dW off 16 bytes", dict(dW_off=8), "misaligned pointer"),
)

# ---- groupnorm_bwd_params (csrc/tune.hip:218 gn_params_blocks: >= 64 rows per block, <= 512 blocks; :173 a block walks its rows across sample-group boundaries) ----
def _gnp(id_, C, groups, rpg, nsg, **kw):
    _add(id_, "gn_params", "gn_params_part_kernel", twice=kw.pop("twice", False), C=C, groups=groups, rpg=rpg, nsg=nsg, **kw)


for _rows, (_rpg, _nsg) in {1: (1, 1), 63: (63, 1), 64: (64, 1), 65: (65, 1), 32704: (511, 64), 32768: (512, 64), 32832: (513, 64)}.items():
    _gnp(f"gnp-rows{_rows}", 64, 32, _rpg, _nsg, silu=_rows % 2 == 1, twice=_rows > 100)     # 1 block; 2 blocks of 33; 511 / 512 blocks of 64; 512 blocks of 65, the last six empty
_gnp("gnp-rpg1", 64, 32, 1, 130, silu=True)                     # 3 blocks of 44 rows, a boundary after every row
_gnp("gnp-rpg-below-block", 64, 32, 10, 13, silu=False)         # blocks of 44 rows straddle four boundaries each, 10 does not divide 44
_gnp("gnp-rpg-equals-block", 64, 32, 64, 2, silu=True)          # rows 128: 2 blocks of 64 = rows_per_group
_gnp("gnp-rpg-above-block", 64, 32, 200, 2, silu=False)         # rows 400: 7 blocks of 58, block 3 straddles the one boundary
_gnp("gnp-rpg-above-block-silu", 320, 32, 97, 3, silu=True)
for _C, _g in ((8, 1), (8, 8), (64, 64), (264, 1), (264, 33), (2560, 32), (2560, 64)):    # one channel per group; 264: the c >= C tail of the second column block
    _gnp(f"gnp-C{_C}-groups{_g}", _C, _g, 37, 3, silu=_g % 2 == 0)
_gnp("gnp-groups1-C64", 64, 1, 70, 2, silu=True)
_gnp("gnp-dgamma-only", 320, 32, 70, 2, silu=True, only="dgamma")
_gnp("gnp-dbeta-only", 320, 32, 70, 2, silu=False, only="dbeta")
_gnp("gnp-alpha", 64, 32, 70, 3, silu=True, alpha=-0.37)
_gnp("gnp-strided", 72, 9, 70, 3, silu=False, dy_pad=4, x_pad=8, alpha=2.0)
_gnp("gnp-prod-L0", 320, 32, 24 * 64 * 64, 1, silu=True, prod=True, twice=True)      # 24 frames of a 64 x 64 latent level: one statistic group, 512 blocks of 192 rows

# ---- refresh_weights (csrc/train.hip:346: one wave per global row, binary search over row0, 256 columns per pass) / refresh_ups4 (csrc/tune.hip:229, grid cap 8192) ----
# an entry: (kind, rows, K[, options]); kind "plain" | "fold" | "fold+bias" | "ups4"; options: m_pad / d_pad widen ld_master / ld_dst
def _rf(id_, entries, **kw):
    # me_refresh_weights (csrc/train.hip:581) does not name its kernel: a table witnesses me_last_kernel only through its folded-upsampler entries, launched last
    _add(id_, "refresh", "refresh_ups4_kernel" if any(e[0] == "ups4" for e in entries) else None, entries=entries, **kw)


for _K in (4, 252, 256, 260):                                   # the 256-column wave loop: one lane, 63 lanes, one full pass, a second pass of one lane
    _rf(f"rf-K{_K}", [("plain", 5, _K), ("fold", 6, _K), ("fold+bias", 3, _K)])
for _r in (4, 5, 7):                                            # total_rows % 4 in {0, 1, 3}: the last block's waves beyond the table
    _rf(f"rf-rows{_r}", [("fold+bias", _r, 72)])
_rf("rf-one-entry-one-row", [("plain", 1, 8)])
_rf("rf-many-one-row-entries", [("plain" if i % 3 else "fold", 1, 40) for i in range(37)])       # every row is a row0 boundary: the search lands on first, last, middle
_rf("rf-mixed", [("plain", 9, 64), ("fold", 1, 320), ("ups4", 10, 24), ("fold+bias", 130, 328), ("plain", 1, 4), ("ups4", 3, 72)])
_rf("rf-strided", [("plain", 6, 72, dict(m_pad=8, d_pad=4)), ("fold+bias", 9, 72, dict(m_pad=4, d_pad=12))])
_rf("rf-ups4-K4", [("ups4", 5, 4)])
_rf("rf-ups4-beyond-the-grid", [("ups4", 2056, 256)])           # 2056 * 16 * 64 = 2,105,344 vectors > 8192 * 256: the loop's second pass, 8192 vectors of it

# ---- conv_small (csrc/eltwise.hip:284 dispatch; :12 direct kernel: 256 pixels x 80-channel slices; :65 tile kernel: 64 pixels x all channels through LDS) ----
_PIX = {1: (1, 1, 1), 63: (1, 7, 9), 64: (1, 8, 8), 65: (1, 5, 13), 255: (1, 15, 17), 256: (2, 8, 16), 257: (1, 1, 257)}     # n_img * H * W -> (n_img, H, W)


def _cs(id_, Cin, Cout, n_img, H, W, **kw):
    _add(id_, "conv_small", conv_small_target(Cin, Cout), Cin=Cin, Cout=Cout, n_img=n_img, H=H, W=W, **kw)


for _Cout in (8, 56, 64, 80, 88, 96, 480, 488, 512):
    for _Cin in (3, 4):
        _cs(f"cs-Cin{_Cin}-Cout{_Cout}", _Cin, _Cout, 1, 5, 13, f16=_Cout % 16 == 0 and _Cin == 4, silu=_Cout in (56, 96, 488))
for _np, (_n, _H, _W) in _PIX.items():
    _cs(f"cs-tile-pix{_np}", 4, 96, _n, _H, _W)
    _cs(f"cs-direct-pix{_np}", 3, 88, _n, _H, _W, silu=True)
_cs("cs-W1", 4, 64, 2, 63, 1)
_cs("cs-W1-direct", 3, 16, 2, 63, 1, f16=True)
_cs("cs-H1-tile", 3, 128, 3, 1, 30, f16=True)
_cs("cs-5d-frames", 4, 320, 6, 6, 5, frames=3)                  # the 5-D latent form: image i at (i / frames) img_stride + (i % frames) frame_stride
_cs("cs-5d-frames-direct-f16", 4, 88, 6, 3, 5, frames=2, f16=True)
_cs("cs-img-stride-wide", 3, 128, 3, 6, 7, img_pad=11)
_cs("cs-img-stride-wide-direct", 4, 8, 3, 6, 7, img_pad=5, silu=True)
_cs("cs-no-bias", 4, 96, 1, 9, 9, bias=False)
_cs("cs-no-bias-direct", 3, 512, 1, 9, 9, bias=False, silu=True)
_cs("cs-prod-conv-in", 4, 320, 24, 64, 64, frames=24, prod=True)

# ---- flat and row-wise kernels (csrc/eltwise.hip:127-185, csrc/clip.hip:11-48: grid_for(n, 16384) blocks, grid-stride loops; 8 halves per thread + a scalar tail) ----
for _r, _id in ((FLAT_EDGE, "at"), (FLAT_EDGE + 1, "above")):      # exactly cap * 256 vectors (one pass) and one more; cols 4 / 8: the narrowest rows that reach the cap
    _add(f"axpy-cap-{_id}", "axpy_rows", "axpy_rows_kernel", rows=_r, cols=4, alpha=0.5)
    _add(f"copy-rows-cap-{_id}", "copy_rows", "copy_rows_kernel", rows=_r, cols=8)
    _add(f"copy-blocks-cap-{_id}", "copy_blocks", "copy_blocks_kernel", n0=1, n1=1, rows=_r, cols=8)
    _add(f"embed-cap-{_id}", "embed_rows", "embed_rows_kernel", rows=_r, seq=64 if _id == "at" else 5, C=8, vocab=11)      # 2^22 + 1 = 5 * 838861
    for _op, _k in (("silu", "unary_kernel<silu>"), ("relu", "unary_kernel<relu>"), ("quick_gelu", "quick_gelu_kernel")):
        _add(f"{_op}-cap-{_id}", _op, _k, n=_r * 8 + (1 if _id == "above" else 0), elementwise=None if _op == "relu" else "f16-out")
for _op, _k in (("silu", "unary_kernel<silu>"), ("relu", "unary_kernel<relu>"), ("quick_gelu", "quick_gelu_kernel")):
    for _n in (1, 7, 8, 9, 2049, 2055):                          # the scalar tail alone, none, one element, 8 k + 1, 8 k + 7 (a second block)
        _add(f"{_op}-n{_n}", _op, _k, n=_n, elementwise=None if _op == "relu" else "f16-out")
    _add(f"{_op}-saturating", _op, _k, n=27, saturating=True, elementwise=None if _op == "relu" else "f16-out")
_add("silu-in-place", "silu", "unary_kernel<silu>", n=1003, inplace=True, elementwise="f16-out")
_add("relu-in-place", "relu", "unary_kernel<relu>", n=1003, inplace=True)
_add("axpy-strided", "axpy_rows", "axpy_rows_kernel", rows=301, cols=68, y_pad=4, x_pad=8, a_pad=12, alpha=-1.5)
_add("axpy-in-place", "axpy_rows", "axpy_rows_kernel", rows=77, cols=320, y_pad=8, x_pad=8, a_pad=4, alpha=0.5, inplace=True)
_add("axpy-one-vector", "axpy_rows", "axpy_rows_kernel", rows=1, cols=4, alpha=1.0)
_add("copy-rows-strided", "copy_rows", "copy_rows_kernel", rows=301, cols=72, y_pad=8, x_pad=16)
_add("copy-rows-one-vector", "copy_rows", "copy_rows_kernel", rows=1, cols=8)
_add("copy-blocks-frame-to-pixel", "copy_blocks", "copy_blocks_kernel", n0=4, n1=6, rows=16, cols=48, x_pad=8, order="to-pixel")     # test_copy_blocks_is_the_frame_pixel_reorder
_add("copy-blocks-pixel-to-frame", "copy_blocks", "copy_blocks_kernel", n0=4, n1=6, rows=16, cols=48, y_pad=8, order="to-frame")
_add("copy-blocks-n0-1", "copy_blocks", "copy_blocks_kernel", n0=1, n1=5, rows=3, cols=8, order="to-pixel")
_add("copy-blocks-n1-1", "copy_blocks", "copy_blocks_kernel", n0=5, n1=1, rows=3, cols=8, y_pad=8, x_pad=8, order="to-frame")
_add("embed-seq-crossed", "embed_rows", "embed_rows_kernel", rows=7 * 77, seq=77, C=8, vocab=300)                # rows cross seq seven times; ids 0 and vocab - 1 among them
_add("embed-C768", "embed_rows", "embed_rows_kernel", rows=3 * 5, seq=5, C=768, vocab=40)
_add("embed-id-out-of-range", "embed_rows", "embed_rows_kernel", rows=4 * 6, seq=6, C=16, vocab=9, bad_ids=True)   # through capi: a zero row, its neighbours right

# ---- step scalars and layouts (csrc/eltwise.hip:188-255: one thread per element, ceil(total / 256) blocks) ----
for _dim in (2, 320, 1280):
    for _t in (0.0, 1.0, 981.0, 999.0):
        _add(f"temb-dim{_dim}-t{int(_t)}", "timestep_embed", "timestep_embed_kernel", rows=3, dim=_dim, t=_t)
for _rows, _dim in ((127, 2), (128, 2), (129, 2), (1, 254), (1, 256), (1, 258)):      # rows * dim around one block of 256
    _add(f"temb-{_rows}x{_dim}", "timestep_embed", "timestep_embed_kernel", rows=_rows, dim=_dim, t=501.0)
for _nb in (1, 2, 3):
    for _g in (0.0, 1.0, 7.5):
        _add(f"ddim-nb{_nb}-g{_g}", "cfg_ddim", "cfg_ddim_kernel", nb=_nb, C=4, f=3, h=5, w=7, guidance=_g, e_pad=4 if _nb == 2 else 0)
_add("ddim-one-block", "cfg_ddim", "cfg_ddim_kernel", nb=1, C=4, f=1, h=8, w=8, guidance=7.5, e_pad=8)          # total = 256 exactly
_add("ddim-C8-lde-wide", "cfg_ddim", "cfg_ddim_kernel", nb=2, C=8, f=3, h=1, w=11, guidance=3.0, e_pad=16)
for _id, _kw in (("plain", dict(n_img=3, npix=35)), ("ldm-wide-scale", dict(n_img=2, npix=64, m_pad=8, scale=0.18215)), ("logvar-clamps", dict(n_img=2, npix=33, m_pad=4, clamps=True, scale=0.5)),
                 ("one-pixel", dict(n_img=1, npix=1))):
    _add(f"gauss-{_id}", "gaussian_sample", "gaussian_sample_kernel", **_kw)
for _C in (3, 4, 8):
    for _np in (1, 85, 256):                                     # npix tails against the 256-thread block
        _add(f"to-rows-C{_C}-npix{_np}", "nchw_to_rows", "nchw_to_rows_kernel", n_img=3, C=_C, npix=_np, y_pad=8 if _np == 85 else 0, img_pad=7 if _np == 85 else 0, ch_pad=3 if _C == 4 else 0)
        _add(f"to-nchw-C{_C}-npix{_np}", "rows_to_nchw", "rows_to_nchw_kernel", n_img=3, C=_C, npix=_np, x_pad=8 if _np != 256 else 0, img_pad=5 if _np == 85 else 0, ch_pad=2 if _C == 3 else 0)
STEP_TWINS = ("timestep_embed", "cfg_ddim")                      # entries with a _dev variant: bitwise the host-scalar launch

# ---- attention_causal (csrc/clip.hip:59: 64-query blocks, 16-key tiles paired into 32-deep contractions, zero padding to nkeys_pad, early return after the barrier) ----
CAUSAL_NQ = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 77, 96, 97, 127, 128)
for _nq in CAUSAL_NQ:
    _add(f"causal-nq{_nq}", "attention_causal", "attn_causal_kernel", twice=True, nq=_nq, heads=1 if _nq % 2 else 12, n_seq=3 if _nq % 2 else 1, kind="soft" if _nq % 3 else "high-gain")
for _kind in ("rising", "falling", "high-gain", "soft"):
    for _nq in (17, 33, 65, 77, 128):
        _add(f"causal-{_kind}-nq{_nq}", "attention_causal", "attn_causal_kernel", twice=True, nq=_nq, heads=12 if _nq == 77 else 2, n_seq=3 if _nq in (33, 77) else 1, kind=_kind,
             separate=_nq in (17, 65), o_pad=8 if _nq != 33 else 0)
_add("causal-scale", "attention_causal", "attn_causal_kernel", twice=True, nq=50, heads=3, n_seq=2, kind="soft", scale=0.3, separate=True, o_pad=16)
CAUSAL_REFUSED = (("dh 40", dict(dh=40), "dh = 64"), ("nq 129", dict(nq=129), "128"), ("ldq % 8", dict(ldq=196), "row strides"), ("ldo < heads dh", dict(ldo=56), "row strides"),
                  ("K off 16 bytes", dict(K_off=8), "row strides"), ("O off 16 bytes", dict(O_off=8), "row strides"), ("scale 0", dict(scale=0.0), "bad arguments"))

BY_ID = {c.id: c for c in CASES}
ENTRIES = sorted({c.entry for c in CASES})


def case_counts() -> Dict[str, int]:
    out: Dict[str, int] = {}
    for c in CASES:
        out[c.entry] = out.get(c.entry, 0) + 1
    return out


def bound_of(case, name) -> Tuple[float, float]:
    if case.bound is not None:
        return case.bound
    return BOUNDS[f"gn_params.{name}"] if case.entry == "gn_params" else BOUNDS[case.entry]


# ---------------------------------------------------------------------------------------------------------------- seeded input builders (CPU tensors)
def _gen(case, salt=""):
    return torch.Generator().manual_seed(seed_of(case.id + salt))


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


_wide = bc._wide
SATURATING = (65504.0, -65504.0, 20.0, -20.0, 0.0, -0.0, 11.0, -11.0, 6.0e-5, -6.0e-5, 1.0)


def build(case) -> dict:
    """The CPU input tensors of a case, fp16 / fp32 as the HIP entry point takes them; operands with a pad are the WIDE allocations, the runner cuts the views."""
    p, g, e = case.p, _gen(case), case.entry
    if e == "conv_dw":
        N, K, M = p["N"], p["K"], p["M"]
        x = _wide(_randn(g, p["n_img"] * p["Hin"] * p["Win"], K).half(), p.get("x_pad", 0), fill=float("nan"))
        dy = _randn(g, M, N)
        dy = _wide(dy.half() if p.get("dy16") else dy, p.get("dy_pad", 0), fill=float("nan"))       # the padding columns must not be read
        return dict(x=x, dy=dy, base=_randn(g, N, 9, K, scale=0.5))
    if e == "gn_params":
        C, rows = p["C"], p["rpg"] * p["nsg"]
        x = (_randn(g, rows, C) * 1.5 + 0.5).half()
        return dict(x=_wide(x, p.get("x_pad", 0), fill=float("nan")), gamma=(1 + 0.2 * _randn(g, C)).half(), beta=(0.2 * _randn(g, C)).half(),
                    dy=_wide(_randn(g, rows, C), p.get("dy_pad", 0), fill=float("nan")), dgamma=_randn(g, C, scale=0.5), dbeta=_randn(g, C, scale=0.5))
    if e == "refresh":
        out = []
        for kind, rows, K, *opt in p["entries"]:
            o = opt[0] if opt else {}
            if kind == "ups4":
                out.append(dict(kind=kind, master=_randn(g, rows, 9, K, scale=0.1), dst=_randn(g, rows, 16, K).half()))
                continue
            d = dict(kind=kind, master=_wide(_randn(g, rows, K, scale=0.05), o.get("m_pad", 0), fill=float("nan")), dst=_wide(_randn(g, rows, K).half(), o.get("d_pad", 0), fill=3.0), K=K)
            if kind != "plain":
                d.update(gamma=1 + 0.1 * _randn(g, K), beta=0.1 * _randn(g, K), colsum=_randn(g, rows), cvec=_randn(g, rows))
            if kind == "fold+bias":
                d["bias"] = _randn(g, rows)
            out.append(d)
        return dict(entries=out)
    if e == "conv_small":
        Cin, Cout, n_img, H, W, frames = p["Cin"], p["Cout"], p["n_img"], p["H"], p["W"], p.get("frames", 0)
        pad = p.get("img_pad", 0)
        if frames:                                               # [B, Cin, frames, H, W]
            inp = _randn(g, n_img // frames, Cin, frames, H, W)
            geo = dict(img_stride=Cin * frames * H * W, ch_stride=frames * H * W, frames=frames, frame_stride=H * W)
        else:                                                    # [n_img, Cin * H * W + pad]: the pad is NaN and never read
            inp = torch.full((n_img, Cin * H * W + pad), float("nan"))
            inp[:, :Cin * H * W] = _randn(g, n_img, Cin * H * W)
            geo = dict(img_stride=Cin * H * W + pad, ch_stride=H * W)
        return dict(inp=inp.half() if p.get("f16") else inp, w=_randn(g, Cout, 9, Cin, scale=0.2), bias=_randn(g, Cout, scale=0.1) if p.get("bias", True) else None, geo=geo)
    if e == "axpy_rows":
        rows, cols = p["rows"], p["cols"]
        x = _wide(_randn(g, rows, cols).half(), p.get("x_pad", 0), fill=float("nan"))
        return dict(x=x, a=_wide(_randn(g, rows, cols).half(), p.get("a_pad", 0), fill=float("nan")))
    if e == "copy_rows":
        return dict(x=_wide(_randn(g, p["rows"], p["cols"]).half(), p.get("x_pad", 0), fill=float("nan")))
    if e == "copy_blocks":
        return dict(x=_wide(_randn(g, p["n0"] * p["n1"] * p["rows"], p["cols"]).half(), p.get("x_pad", 0), fill=float("nan")))
    if e in ("silu", "relu", "quick_gelu"):
        n = p["n"]
        if p.get("saturating"):
            x = torch.cat([torch.tensor(SATURATING), _randn(g, n - len(SATURATING), scale=3.0)])
        else:
            x = _randn(g, n, scale=2.0)
            x[:min(n, 64)] = torch.linspace(-30.0, 30.0, 64)[:min(n, 64)]         # both tails of the sigmoid
            x[-1] = -4.0                                                          # the last element (the scalar tail's, where there is one) is not a zero
        return dict(x=x.half())
    if e == "embed_rows":
        rows, seq, C, vocab = p["rows"], p["seq"], p["C"], p["vocab"]
        ids = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
        ids[0], ids[-1], ids[rows // 2] = 0, vocab - 1, vocab - 1
        if p.get("bad_ids"):
            ids[3], ids[seq], ids[-2] = vocab, -1, 1 << 30
        return dict(tok=_randn(g, vocab, C).half(), pos=_randn(g, seq + 2, C, scale=0.25).half(), ids=ids)
    if e == "timestep_embed":
        return {}
    if e == "cfg_ddim":
        nb, C, f, h, w = p["nb"], p["C"], p["f"], p["h"], p["w"]
        return dict(lat=_randn(g, nb, C, f, h, w), eps=_wide(_randn(g, 2 * nb * f * h * w, C).half(), p.get("e_pad", 0), fill=float("nan")), ca=1.01, cb=-0.07)
    if e == "gaussian_sample":
        n_img, npix = p["n_img"], p["npix"]
        mom = _randn(g, n_img * npix, 8)
        if p.get("clamps"):                                      # logvar at and beyond -30 and 20
            mom[:8, 4:] = torch.tensor([-30.0, -30.02, -45.0, -60000.0, 20.0, 20.02, 31.0, 60000.0])[:, None]
            mom[:8, :4] = 0.5
        return dict(mom=_wide(mom.half(), p.get("m_pad", 0), fill=float("nan")), noise=_randn(g, n_img, 4, npix))
    if e == "nchw_to_rows":
        n_img, C, npix = p["n_img"], p["C"], p["npix"]
        chs = npix + p.get("ch_pad", 0)
        x = torch.full((n_img, C * chs + p.get("img_pad", 0)), float("nan"))
        for c in range(C):
            x[:, c * chs:c * chs + npix] = _randn(g, n_img, npix, scale=2.0)
        return dict(x=x, img_stride=x.shape[1], ch_stride=chs)
    if e == "rows_to_nchw":
        return dict(x=_wide(_randn(g, p["n_img"] * p["npix"], p["C"], scale=2.0).half(), p.get("x_pad", 0), fill=float("nan")))
    if e == "attention_causal":
        nq, heads, n_seq, kind = p["nq"], p["heads"], p["n_seq"], p["kind"]
        C, scale = heads * 64, p.get("scale") or 0.125
        qkv = _randn(g, n_seq * nq, 3 * C, scale=0.7)
        if kind == "high-gain":                                  # tests/test_clip_gpu.py test_attn_causal: logits of std ~ 9 before the mask
            qkv = _randn(_gen(case, "/hg"), n_seq * nq, 3 * C)
            qkv[:, :2 * C] *= 3.0
        elif kind in ("rising", "falling"):                      # tests/long_clip_cases.py: + / - 0.25 j on the score of key j along a unit direction per head
            u = _randn(_gen(case, "/direction"), heads, 64)
            u = u / u.norm(dim=1, keepdim=True)
            q = qkv[:, :C].reshape(n_seq, nq, heads, 64) + 4.0 * u
            shift = (1.0 if kind == "rising" else -1.0) * 0.25 * torch.arange(nq, dtype=torch.float32) / (4.0 * scale)
            k = qkv[:, C:2 * C].reshape(n_seq, nq, heads, 64) + shift[None, :, None, None] * u
            qkv = torch.cat([q.reshape(-1, C), k.reshape(-1, C), qkv[:, 2 * C:]], dim=1)
        return dict(qkv=qkv.half())
    raise KeyError(e)
