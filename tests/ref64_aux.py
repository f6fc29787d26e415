"""TEST INFRASTRUCTURE: the entry points of the third sweep (tests/aux_cases.py) stated in plain double precision, for the operations tests/ref64_bwd.py and
tests/ref64_fwd.py have no statement of.  Every function has the signature of its ``motioneditor_amd.ops`` namesake and returns fp64 (copies and selections keep
the dtype), so one case table drives the HIP library, the fp32 emulation and this reference alike.  Nothing here goes through tests/emu_ops.py: explicit tap
loops, no F.conv2d / F.silu / torch.softmax.  gemm_dw(conv=...) is tests/ref64_bwd.py's; the GroupNorm affine gradients are autograd of its fp64 forward."""
from __future__ import annotations

import math

import torch

import ref64_bwd
from ref64_bwd import D, _d, gemm_dw  # noqa: F401


def groupnorm_bwd(x, gamma, beta, dy, *, rows_per_group, eps, silu, groups=32, dgamma=None, dbeta=None):
    """dgamma / dbeta (fp64 [C], either may be None) are ACCUMULATED into; dx is not what the sweep is about and is not returned."""
    g0, b0 = _d(gamma).clone().requires_grad_(True), _d(beta).clone().requires_grad_(True)
    y = ref64_bwd._groupnorm(_d(x), g0, b0, rows_per_group=rows_per_group, eps=eps, silu=silu, groups=groups)
    dg, db = torch.autograd.grad(y, (g0, b0), _d(dy))
    if dgamma is not None:
        dgamma += dg
    if dbeta is not None:
        dbeta += db


def _sigmoid(x):
    return 1.0 / (1.0 + (-x).exp())


def conv_small(inp, w, bias, *, n_img, Cin, H, Wd, img_stride, ch_stride, frames=0, frame_stride=0, silu=False):
    """me_conv_small: 3 x 3, pad 1, on planar images addressed by strides; w [Cout, 9, Cin] fp32, rows out [(n_img H Wd), Cout]."""
    flat, w = _d(inp).reshape(-1), _d(w)
    Cout = w.shape[0]
    pad = torch.zeros((n_img, Cin, H + 2, Wd + 2), dtype=D)
    for i in range(n_img):
        base = (i // frames) * img_stride + (i % frames) * frame_stride if frames > 0 else i * img_stride
        for c in range(Cin):
            pad[i, c, 1:-1, 1:-1] = flat[base + c * ch_stride:base + c * ch_stride + H * Wd].reshape(H, Wd)
    y = torch.zeros((n_img, H, Wd, Cout), dtype=D) if bias is None else _d(bias).expand(n_img, H, Wd, Cout).clone()
    for ky in range(3):
        for kx in range(3):
            y = y + pad[:, :, ky:ky + H, kx:kx + Wd].permute(0, 2, 3, 1) @ w[:, ky * 3 + kx].t()
    if silu:
        y = y * _sigmoid(y)
    return y.reshape(-1, Cout)


def axpy_rows(y, x, a_, alpha=1.0):
    y.copy_(_d(x) + alpha * _d(a_))
    return y


def copy_rows(y, x):
    y.copy_(x)
    return y


def copy_blocks(y, x, n0, n1, rows, *, ys0, ys1, xs0, xs1):
    for i in range(n0):
        for j in range(n1):
            y[i * ys0 + j * ys1:i * ys0 + j * ys1 + rows, :x.shape[1]] = x[i * xs0 + j * xs1:i * xs0 + j * xs1 + rows]
    return y


def silu(x):
    x = _d(x)
    return x * _sigmoid(x)


def relu(x):
    return torch.where(x > 0, x, torch.zeros((), dtype=x.dtype))


def quick_gelu(x):
    x = _d(x)
    return x * _sigmoid(1.702 * x)


def embed_rows(tok, pos, ids, seq):
    """out[r] = f16(tok[ids[r]] + pos[r % seq]); an id outside [0, vocab) leaves a zero row (csrc/clip.hip embed_rows_kernel)."""
    ids = ids.reshape(-1).long()
    ok = (ids >= 0) & (ids < tok.shape[0])
    r = torch.arange(ids.numel())
    s = _d(tok)[ids.clamp(0, tok.shape[0] - 1)] + _d(pos)[r % seq]
    return torch.where(ok[:, None], s, torch.zeros((), dtype=D)).to(tok.dtype)


def timestep_embed(rows, dim, t, device=None):
    half = dim // 2
    ang = float(t) * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=D) / half)
    return torch.cat([torch.cos(ang), torch.sin(ang)])[None].repeat(rows, 1)


def cfg_ddim(latents, eps_rows, *, guidance, ca, cb):
    """The scalars are the fp32 values me_cfg_ddim's signature carries."""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))    # noqa: E731
    nb, C, f, h, w = latents.shape
    e = _d(eps_rows)[:, :C].reshape(2 * nb, f, h * w, C).permute(0, 3, 1, 2).reshape(2 * nb, C, f, h, w)
    eu, ec = e[:nb], e[nb:]
    return f32(ca) * _d(latents) + f32(cb) * (eu + f32(guidance) * (ec - eu))


def gaussian_sample(moments, noise, n_img, npix, scale=1.0):
    m = _d(moments)[:, :8].reshape(n_img, npix, 8).permute(0, 2, 1)
    return (m[:, :4] + torch.exp(0.5 * m[:, 4:].clamp(-30.0, 20.0)) * _d(noise).reshape(n_img, 4, npix)) * float(torch.tensor(scale, dtype=torch.float32))


def nchw_to_rows(x, n_img, C, npix, img_stride, ch_stride):
    flat = _d(x).reshape(-1)
    out = torch.empty((n_img * npix, C), dtype=D)
    for i in range(n_img):
        for c in range(C):
            out[i * npix:(i + 1) * npix, c] = flat[i * img_stride + c * ch_stride:i * img_stride + c * ch_stride + npix]
    return out


def rows_to_nchw(x, n_img, C, npix):
    return _d(x)[:, :C].reshape(n_img, npix, C).permute(0, 2, 1).contiguous()


def attention_causal(q, k, v, *, heads, dh, n_seq, nq, scale=None):
    scale = dh ** -0.5 if scale is None else scale
    sp = lambda t: _d(t)[:n_seq * nq, :heads * dh].reshape(n_seq, nq, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
    s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
    s = s.masked_fill(torch.arange(nq)[None, :] > torch.arange(nq)[:, None], -math.inf)
    e = (s - s.max(dim=-1, keepdim=True).values).exp()
    return ((e / e.sum(dim=-1, keepdim=True)) @ sp(v)).permute(0, 2, 1, 3).reshape(n_seq * nq, heads * dh)


def refresh_entry(d):
    """One entry of a refresh table from its fp32 values: what weights.Packed builds.  plain: f16(master); fold: W' is weights.Packed.ln_fold's own tensor (f16 of
    the fp32 product master * gamma), colsum over that ROUNDED W' and cvec = master beta + bias are taken in fp64 here; ups4: Packed.fold_ups, rounded once."""
    from motioneditor_amd.weights import Packed
    m = d["master"]
    if d["kind"] == "ups4":
        n, _, k = m.shape
        return dict(w=Packed.fold_ups(m.reshape(n, 3, 3, k).permute(0, 3, 1, 2).contiguous()).half())
    m = m[:, :d["K"]]
    if d["kind"] == "plain":
        return dict(w=m.half())
    st = {"w": m.contiguous(), "n.weight": d["gamma"], "n.bias": d["beta"]}
    wq = Packed(st, "cpu").ln_fold("n", ["w"])[0][:, 0, :]
    cvec = m.double() @ d["beta"].double()
    return dict(w=wq, colsum=wq.double().sum(dim=1), cvec=cvec + d["bias"].double() if d.get("bias") is not None else cvec)
