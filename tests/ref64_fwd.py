"""TEST INFRASTRUCTURE: the forward family of include/motioned.h (me_gemm, me_attn, me_tattn, me_groupnorm, me_layernorm, me_softmax_rows, me_ln_stats) stated
in plain double precision, on the forward helpers tests/ref64_bwd.py already holds (_gather_gemm, _groupnorm, _layernorm, _gelu).

Every function has the signature of its ``motioneditor_amd.ops`` (and ``tests/emu_ops.py``) namesake, so one case table (tests/fwd_cases.py) drives the HIP
library, the fp32 emulation and this reference alike.  Nothing here goes through emu_ops.  Inputs are the fp16 (or, for the LayerNorm fold's statistics and
vectors, fp32) values the kernel is given, widened to fp64; all arithmetic is fp64 and NOTHING is rounded on the way: the fp16 roundings the me_gemm
contract performs between its epilogue terms (include/motioned.h: without an activation the tile is rounded before rowvec / res / res2 are added in fp16)
are at most three relative errors of 2^-11 on the result and are charged to the entry point's bound, as the fp16 rounding of every output is.  Two places
read a ROUNDED value because the contract defines them on one: `ln_out` is the row sums of the fp16 output rows the launch stored (tests/fwd_run.py takes
them from the output under test), and ups = 3 is referenced from the folded [N, 16, K] fp16 weights the kernel is given, so the fold's own rounding is not
charged to the kernel.  GEGLU: include/motioned.h states value * gelu(gate) with the erf GELU and no intermediate rounding."""
from __future__ import annotations

import math

import torch

from ref64_bwd import D, _d, _gather_gemm, _gelu, _groupnorm, _layernorm

SEG_PLAIN, SEG_DUAL_CUR, SEG_DUAL_PREV, SEG_DUAL_BIN = 0, 1, 2, 3
LOG2E = 1.4426950408889634


def _row_parts(y):
    """[P, rows, 2] (sum, sum of squares) over 320-column parts: the me_gemm_args.ln_stats / ln_out format."""
    rows, C = y.shape
    P = C // 320 if C % 320 == 0 else 1
    t = _d(y).reshape(rows, P, C // P)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], dim=-1).permute(1, 0, 2).contiguous()


def ln_stats(x):
    return _row_parts(x)


def gemm(x, w, *, M=None, out=None, bias=None, rowvec=None, rows_per_vec=0, res=None, res2=None, geglu=False, act=0, alpha=1.0, conv=None, tconv=None,
         res_rows=0, res2_rows=0, head_major=None, row_range=None, ln=None, ln_out=False):
    """me_gemm: gather (dense; conv 3 x 3 with stride 1 | 2, ups 0 | 1 | 3, pad0; tconv with chunk, frame0, frames_total and halos), then the epilogue in the
    order of include/motioned.h: alpha, the LayerNorm fold, bias, [GEGLU |] rowvec, act, res, res2; head_major = (col0, dh) splits the columns from col0 on
    into [heads, M, dh] panels; row_range = (lo, hi) writes rows [lo, hi) of the full problem into `out`; ln_out returns (y, row sums of y)."""
    N, taps, K = w.shape
    if M is None:
        M = x.shape[0]
    acc = _gather_gemm(_d(x), _d(w), M=M, alpha=alpha, conv=conv, tconv=tconv)
    if ln is not None:
        st, colsum, cvec, eps = ln
        S = _d(st).sum(dim=0)[:M]
        mean = S[:, 0] / K
        rstd = ((S[:, 1] / K - mean * mean).clamp_min(0) + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()
        acc = rstd[:, None] * (acc - mean[:, None] * _d(colsum)[None]) + _d(cvec)[None]
    if bias is not None:
        acc = acc + _d(bias)
    if geglu:
        q = acc.reshape(M, N // 32, 2, 16)
        y = (q[:, :, 0] * _gelu(q[:, :, 1])).reshape(M, N // 2)
    else:
        y = acc
        if rowvec is not None:
            y = y + _d(rowvec)[torch.arange(M) // rows_per_vec][:, :N]
        if act == 1:
            y = y.clamp_min(0)
        elif act == 2:
            y = y / (1.0 + (-y).exp())
        if res is not None:
            y = y + _d(res)[(torch.arange(M) % res_rows) if res_rows else slice(0, M), :N]
        if res2 is not None:
            y = y + _d(res2)[(torch.arange(M) % res2_rows) if res2_rows else slice(0, M), :N]
    if row_range is not None:
        lo, hi = row_range
        out[lo:hi, :y.shape[1]] = y[lo:hi]
        return out[:M, :y.shape[1]]
    if head_major is not None:
        col0, dh = head_major
        panels = y[:, col0:].reshape(M, (N - col0) // dh, dh).permute(1, 0, 2).contiguous()
        return (y[:, :col0] if col0 else None), panels
    if out is not None:
        out[:M, :y.shape[1]] = y
        y = out[:M, :y.shape[1]]
    return (y, _row_parts(y.to(torch.float16))) if ln_out else y


def _rows(t, heads, dh):
    """Head-major [heads, rows, dh] panels (me_attn_args.hsq / hsk / hsv) as rows [rows, heads * dh]."""
    t = _d(t)
    return t.permute(1, 0, 2).reshape(t.shape[1], heads * dh) if t.dim() == 3 else t[:, :heads * dh]


def _logits_values(q, k, v, *, heads, dh, n_items, nq, nk, seg_item, seg_mode, mask, scale, q_items):
    """Per item: the logits [heads, nq, keys] and values [heads, keys, dh] of every key copy of its segment list (a negative entry closes the list)."""
    q, k, v = _rows(q, heads, dh), _rows(k, heads, dh), _rows(v, heads, dh)
    si, sm = seg_item.tolist(), seg_mode.tolist()
    mk = None if mask is None else _d(mask)
    for it in range(n_items):
        iq = it % q_items if q_items else it
        qi = q[iq * nq:(iq + 1) * nq].reshape(nq, heads, dh).permute(1, 0, 2)
        logits, vals = [], []
        for s, kit in enumerate(si[it]):
            if kit < 0:
                break
            ks = k[kit * nk:(kit + 1) * nk].reshape(nk, heads, dh).permute(1, 0, 2)
            vs = v[kit * nk:(kit + 1) * nk].reshape(nk, heads, dh).permute(1, 0, 2)
            sc = (qi @ ks.transpose(1, 2)) * scale
            mode = sm[it][s]
            if mode == SEG_PLAIN:
                logits.append(sc)
                vals.append(vs)
            elif mode == SEG_DUAL_BIN:                   # weight exp(s) + 1 whatever the mask bit says: the second copy has logit 0 and the same V
                logits += [sc, torch.zeros_like(sc)]
                vals += [vs, vs]
            else:                                        # DUAL_CUR reads mask plane `head`, DUAL_PREV plane max(head - 1, 0)
                planes = torch.tensor([h if mode == SEG_DUAL_CUR else max(h - 1, 0) for h in range(heads)])
                m = mk[planes][:, None, :nk]
                logits += [sc * m, sc * (1 - m)]
                vals += [vs, vs]
        yield it, torch.cat(logits, dim=-1), torch.cat(vals, dim=1)


def attention(q, k, v, *, heads, dh, n_items, nq, nk, seg_item, seg_mode, mask=None, scale=None, out=None, q_items=0, lse=None):
    scale = dh ** -0.5 if scale is None else scale
    C = heads * dh
    res = torch.empty((n_items * nq, C), dtype=D)
    for it, lg, vals in _logits_values(q, k, v, heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, seg_item=seg_item, seg_mode=seg_mode, mask=mask, scale=scale,
                                       q_items=q_items):
        if lse is not None:
            lse[it * nq:(it + 1) * nq] = (torch.logsumexp(lg, dim=-1) * LOG2E).t()
        e = (lg - lg.max(dim=-1, keepdim=True).values).exp()
        p = e / e.sum(dim=-1, keepdim=True)
        res[it * nq:(it + 1) * nq] = (p @ vals).permute(1, 0, 2).reshape(nq, C)
    if out is not None:
        out[:, :C] = res
        return out
    return res


def attention_lse(q, k, *, heads, dh, n_items, nq, nk, seg_item, seg_mode=None, scale=None, q_items=0):
    """The log2-domain log-sum-exp [n_items * nq, heads] the forward stashes (plain segments)."""
    lse = torch.empty((n_items * nq, heads), dtype=D)
    sm = torch.zeros_like(seg_item) if seg_mode is None else seg_mode
    attention(q, k, k, heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, seg_item=seg_item, seg_mode=sm, scale=scale, q_items=q_items, lse=lse)
    return lse


def temporal_attention(q, k, v, *, heads, dh, batch, frames, npix, kv_map=None, scale=None, q_frames=0, q_frame0=0, kv_parts=1, q_parts=1):
    """me_tattn: for batch entry b, K / V come from entry kv_map[b]; key frame <= query frame; q holds q_frames frames from global frame q_frame0; K / V
    (and, with q_parts > 1, Q and O) are part-major: row of (b, frame j, p) = ((j / fpp) * batch + b) * fpp * npix + (j % fpp) * npix + p."""
    scale = dh ** -0.5 if scale is None else scale
    C = heads * dh
    km = list(kv_map) if kv_map is not None else list(range(batch))
    qf = q_frames or frames
    parts = max(kv_parts, 1)
    fpp = frames // parts

    def part_major(t):
        t = _d(t)[:, :C].reshape(parts, batch, fpp, npix, heads, dh).permute(1, 0, 2, 3, 4, 5).reshape(batch, frames, npix, heads, dh)
        return t.permute(0, 2, 3, 1, 4)                                      # [b, p, h, f, d]

    qq = part_major(q) if q_parts > 1 else _d(q)[:, :C].reshape(batch, qf, npix, heads, dh).permute(0, 2, 3, 1, 4)
    kk, vv = part_major(k)[km], part_major(v)[km]
    s = (qq @ kk.transpose(-1, -2)) * scale
    gi = (q_frame0 if q_frames else 0) + torch.arange(qf)
    s = s.masked_fill(torch.arange(frames)[None, :] > gi[:, None], -math.inf)
    e = (s - s.max(dim=-1, keepdim=True).values).exp()
    o = (e / e.sum(dim=-1, keepdim=True)) @ vv                               # [b, p, h, qf, d]
    if q_parts > 1:
        o = o.permute(0, 3, 1, 2, 4).reshape(batch, q_parts, fpp, npix, C).permute(1, 0, 2, 3, 4)
        return o.reshape(batch * frames * npix, C)
    return o.permute(0, 3, 1, 2, 4).reshape(batch * qf * npix, C)


def groupnorm(x, gamma, beta, *, rows_per_group, eps, silu, groups=32, out=None, reduce=None, rows_per_group_total=None):
    """me_groupnorm; with `reduce` the split me_groupnorm_stats + me_groupnorm_apply: the hook sees fp64 (sum, sum of squares) per (sample group, channel
    group) and the count is rows_per_group_total * C / groups."""
    x = _d(x)
    if reduce is None:
        return _groupnorm(x, _d(gamma), _d(beta), rows_per_group=rows_per_group, eps=eps, silu=silu, groups=groups)
    rows, C = x.shape
    t = x.reshape(rows // rows_per_group, rows_per_group, groups, C // groups)
    st = torch.stack([t.sum(dim=(1, 3)), (t * t).sum(dim=(1, 3))], dim=-1).reshape(-1).contiguous()
    reduce(st)
    st = st.reshape(rows // rows_per_group, groups, 2)
    cnt = float((rows_per_group_total or rows_per_group) * (C // groups))
    mean = (st[..., 0] / cnt)[:, None, :, None]
    var = (st[..., 1] / cnt)[:, None, :, None] - mean * mean
    y = ((t - mean) / (var + eps).sqrt()).reshape(rows, C) * _d(gamma) + _d(beta)
    return y / (1.0 + (-y).exp()) if silu else y


def layernorm(x, gamma, beta, eps=1e-5):
    return _layernorm(_d(x), _d(gamma), _d(beta), eps)


def softmax_rows(x, out=None):
    x = _d(x)
    e = (x - x.max(dim=-1, keepdim=True).values).exp()
    y = e / e.sum(dim=-1, keepdim=True)
    if out is not None:
        out.copy_(y)
        return out
    return y
