"""TEST INFRASTRUCTURE: the backward / training family of include/motioned.h stated in plain double precision.

Every function has the signature of its ``motioneditor_amd.ops`` (and ``tests/emu_ops.py``) namesake, so one case table (tests/bwd_cases.py) drives the
HIP library, the fp32 emulation and this reference alike.  Nothing here goes through emu_ops: that file stays the independent fp32 statement, and
tests/test_bwd_sweep_cpu.py pins the two against each other.  Operations that are vector-Jacobian products are taken with torch autograd through an
fp64 forward written here from the header (explicit tap loops, no F.conv* / F.layer_norm / F.group_norm); the optimiser and the reductions are written out.

The ops.py contract is kept: entries with ``dst`` / ``dq, dk, dv`` ACCUMULATE (the caller hands fp64 tensors), and ``dy`` is rounded to fp16 where
ops.py does so before the MFMA (gemm_dx: me_cast_rows_f16 in front of me_gemm; gemm_dw: the kernel's own fp32 -> fp16 staging)."""
from __future__ import annotations

import math

import torch

D = torch.float64


def _d(t):
    return t.detach().to(D)


def _leaf(t):
    return t.detach().to(D).clone().requires_grad_(True)


def _r16(t):
    """fp32 gradient -> the fp16 value the MFMA sees, as fp64."""
    return t.detach().to(torch.float32).to(torch.float16).to(D)


# ------------------------------------------------------------------------------------------------------------------ forwards (fp64, differentiable)
def _gather_gemm(x, w, *, M, alpha=1.0, conv=None, tconv=None):
    """y[:M] = alpha * gather(x) @ w^T of me_gemm: w [N, taps, K]; conv = (Hin, Win, Hout, Wout, stride, ups) is the 3 x 3, pad-1 convolution on channels-last
    rows (ups = 1: over the nearest-2x upsample of the input); tconv = (frames, npix, chunk) the 3-tap TemporalConv whose taps stay inside a chunk of frames.
    The forward sweep (tests/ref64_fwd.py) adds: conv[6] = pad0 (1: no padding at the top / left), ups = 3 (w [N, 16, K]: the four 2x2-tap convolutions of
    the folded nearest-2x form, one per output parity) and the frame-sharded tconv = (frames, npix, chunk, frame0, frames_total, halo_prev, halo_next)."""
    N, taps, K = w.shape
    x = x[:, :K]
    if conv is not None and conv[5] == 3:
        Hin, Win, Hout, Wout = conv[:4]
        n_img = x.shape[0] // (Hin * Win)
        img = x[:n_img * Hin * Win].reshape(n_img, Hin, Win, K)
        pad = torch.zeros((n_img, Hin + 2, Win + 2, K), dtype=D)
        pad[:, 1:-1, 1:-1] = img                                   # padded pixel (y + 1, x + 1) = pixel (y, x)
        y = torch.zeros((n_img, Hout, Wout, N), dtype=D)
        for py in range(2):
            for px in range(2):
                for ty in range(2):
                    for tx in range(2):                            # tap (ty, tx) of parity (py, px) reads pixel (y + py - 1 + ty, x + px - 1 + tx)
                        y[:, py::2, px::2] += pad[:, py + ty:py + ty + Hin, px + tx:px + tx + Win] @ w[:, 4 * (2 * py + px) + 2 * ty + tx].t()
        y = y.reshape(-1, N)
    elif conv is not None:
        Hin, Win, Hout, Wout, stride, ups = conv[:6]
        pad0 = conv[6] if len(conv) > 6 else 0
        n_img = x.shape[0] // (Hin * Win)
        img = x[:n_img * Hin * Win].reshape(n_img, Hin, Win, K)
        if ups == 1:
            img = img.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        Hv, Wv = img.shape[1], img.shape[2]
        pad = torch.cat([torch.zeros((n_img, 1, Wv, K), dtype=D), img, torch.zeros((n_img, 1, Wv, K), dtype=D)], dim=1)
        pad = torch.cat([torch.zeros((n_img, Hv + 2, 1, K), dtype=D), pad, torch.zeros((n_img, Hv + 2, 1, K), dtype=D)], dim=2)
        if pad0:                                                   # F.pad(x, (0, 1, 0, 1)): the window starts at the pixel itself
            pad = pad[:, 1:, 1:]
        y = None
        for ky in range(3):
            for kx in range(3):
                sl = pad[:, ky:ky + stride * (Hout - 1) + 1:stride, kx:kx + stride * (Wout - 1) + 1:stride]
                t = sl @ w[:, ky * 3 + kx].t()
                y = t if y is None else y + t
        y = y.reshape(-1, N)
    elif tconv is not None and len(tconv) > 3:
        frames, npix, chunk, frame0, ftot, hp, hn = tconv
        nb = M // (frames * npix)
        t = x[:nb * frames * npix].reshape(nb, frames, npix, K)
        outs = []
        for fr in range(frames):
            acc = torch.zeros((nb, npix, N), dtype=D)
            for tap in range(3):
                gs, ls = frame0 + fr + tap - 1, fr + tap - 1
                if gs < 0 or gs >= ftot or gs // chunk != (frame0 + fr) // chunk:
                    continue
                if 0 <= ls < frames:
                    acc = acc + t[:, ls] @ w[:, tap].t()
                elif (hp if ls < 0 else hn) >= 0:                  # the one-frame halo appended to x (no halo given: the tap contributes nothing)
                    h0 = hp if ls < 0 else hn
                    acc = acc + x[h0:h0 + nb * npix].reshape(nb, npix, K) @ w[:, tap].t()
            outs.append(acc)
        y = torch.stack(outs, dim=1).reshape(-1, N)
    elif tconv is not None:
        frames, npix, chunk = tconv[:3]
        nb = x.shape[0] // (frames * npix)
        t = x[:nb * frames * npix].reshape(nb, frames, npix, K)
        outs = []
        for fr in range(frames):
            acc = torch.zeros((nb, npix, N), dtype=D)
            for tap in range(3):
                fs = fr + tap - 1
                if 0 <= fs < frames and fs // chunk == fr // chunk:
                    acc = acc + t[:, fs] @ w[:, tap].t()
            outs.append(acc)
        y = torch.stack(outs, dim=1).reshape(-1, N)
    else:
        y = x @ w[:, 0].t()
    return alpha * y[:M]


def _attention(q, k, v, *, heads, dh, n_items, nq, nk, seg_item, scale):
    """me_attn for PLAIN segments: item i's queries attend over the concatenated keys of the kv items seg_item[i] lists (a negative entry closes the list)."""
    C = heads * dh
    rows = []
    for it in range(n_items):
        qi = q[it * nq:(it + 1) * nq, :C].reshape(nq, heads, dh).permute(1, 0, 2)
        ks, vs = [], []
        for kit in seg_item[it]:
            if kit < 0:
                break
            ks.append(k[kit * nk:(kit + 1) * nk, :C].reshape(nk, heads, dh).permute(1, 0, 2))
            vs.append(v[kit * nk:(kit + 1) * nk, :C].reshape(nk, heads, dh).permute(1, 0, 2))
        kk, vv = torch.cat(ks, dim=1), torch.cat(vs, dim=1)
        s = (qi @ kk.transpose(1, 2)) * scale
        s = s - s.max(dim=-1, keepdim=True).values.detach()
        e = s.exp()
        p = e / e.sum(dim=-1, keepdim=True)
        rows.append((p @ vv).permute(1, 0, 2).reshape(nq, C))
    return torch.cat(rows, dim=0)


def _tattn(q, k, v, *, heads, dh, batch, frames, npix, scale):
    """me_tattn, plain row order (b f p): every (batch entry, pixel, head) attends causally over the frames."""
    C = heads * dh
    shp = lambda t: t[:, :C].reshape(batch, frames, npix, heads, dh).permute(0, 2, 3, 1, 4)   # noqa: E731   [b, p, h, f, d]
    s = (shp(q) @ shp(k).transpose(-1, -2)) * scale
    future = torch.arange(frames)[None, :] > torch.arange(frames)[:, None]
    s = s.masked_fill(future, -math.inf)
    s = s - s.max(dim=-1, keepdim=True).values.detach()
    e = s.exp()
    p = e / e.sum(dim=-1, keepdim=True)
    return (p @ shp(v)).permute(0, 3, 1, 2, 4).reshape(batch * frames * npix, C)


def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476))


def _groupnorm(x, gamma, beta, *, rows_per_group, eps, silu, groups):
    rows, C = x.shape
    t = x.reshape(rows // rows_per_group, rows_per_group, groups, C // groups)
    mean = t.sum(dim=(1, 3), keepdim=True) / (rows_per_group * (C // groups))
    var = ((t - mean) ** 2).sum(dim=(1, 3), keepdim=True) / (rows_per_group * (C // groups))
    y = ((t - mean) / (var + eps).sqrt()).reshape(rows, C) * gamma + beta
    return y / (1.0 + (-y).exp()) if silu else y


def _layernorm(x, gamma, beta, eps):
    mean = x.sum(dim=1, keepdim=True) / x.shape[1]
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / x.shape[1]
    return (x - mean) / (var + eps).sqrt() * gamma + beta


# ------------------------------------------------------------------------------------------------------------------ the entry points
def grad_acc(dst, src, alpha=1.0, pool=None, store=False):
    if store:
        dst.zero_()
    s = _d(src)
    if pool is not None:
        H, W = pool
        s = s.reshape(-1, H, 2, W, 2, s.shape[-1]).sum(dim=(2, 4)).reshape(-1, s.shape[-1])
    if dst.dim() == 2:
        dst += alpha * s[:dst.shape[0], :dst.shape[1]]
    else:
        dst += alpha * s.reshape(dst.shape)
    return dst


def gemm_dx(dy, w, *, dst, M, alpha=1.0, conv=None, tconv=None, store=False):
    if store:
        dst.zero_()
    x0 = torch.zeros((dst.shape[0], w.shape[2]), dtype=D, requires_grad=True)
    y = _gather_gemm(x0, _d(w), M=M, alpha=alpha, conv=conv, tconv=tconv)
    dst += torch.autograd.grad(y, x0, _r16(dy)[:y.shape[0], :y.shape[1]])[0]
    return dst


def gemm_dw(dy, x, *, dst, taps, K, M, alpha=1.0, conv=None, tconv=None):
    N = dy.shape[1]
    w0 = torch.zeros((N, taps, K), dtype=D, requires_grad=True)
    y = _gather_gemm(_d(x), w0, M=M, alpha=alpha, conv=conv, tconv=tconv)
    dst += torch.autograd.grad(y, w0, _r16(dy)[:y.shape[0], :y.shape[1]])[0]
    return dst


def colsum_grad(dy, *, dst, alpha=1.0):
    dst += alpha * _d(dy).sum(dim=0)
    return dst


def geglu_bwd(pre, dy):
    p0 = _leaf(pre)
    M, N = p0.shape
    q = p0.reshape(M, N // 32, 2, 16)
    y = (q[:, :, 0] * _gelu(q[:, :, 1])).reshape(M, N // 2)
    return torch.autograd.grad(y, p0, _d(dy))[0]


def attention_bwd(q, k, v, out, dout, *, dq, dk, dv, lse=None, heads, dh, n_items, nq, nk, seg_item, seg_mode=None, mask=None, scale=None, q_items=0):
    assert mask is None and not q_items
    q0, k0, v0 = _leaf(q), _leaf(k), _leaf(v)
    y = _attention(q0, k0, v0, heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, seg_item=seg_item.tolist(), scale=dh ** -0.5 if scale is None else scale)
    gq, gk, gv = torch.autograd.grad(y, (q0, k0, v0), _d(dout)[:, :heads * dh])
    dq += gq[:, :dq.shape[1]]
    dk += gk[:, :dk.shape[1]]
    dv += gv[:, :dv.shape[1]]


def attention_lse(q, k, *, heads, dh, n_items, nq, nk, seg_item, scale=None):
    """The log2-domain log-sum-exp [n_items * nq, heads] the forward stashes for its backward."""
    scale = dh ** -0.5 if scale is None else scale
    C = heads * dh
    q, k = _d(q), _d(k)
    rows = []
    for it in range(n_items):
        qi = q[it * nq:(it + 1) * nq, :C].reshape(nq, heads, dh).permute(1, 0, 2)
        kk = torch.cat([k[kit * nk:(kit + 1) * nk, :C].reshape(nk, heads, dh).permute(1, 0, 2) for kit in seg_item.tolist()[it] if kit >= 0], dim=1)
        rows.append((torch.logsumexp((qi @ kk.transpose(1, 2)) * scale, dim=-1) * 1.4426950408889634).t())
    return torch.cat(rows, dim=0)


def temporal_attention_bwd(q, k, v, out, dout, *, heads, dh, batch, frames, npix, scale=None, **kw):
    assert not any(kw.get(n) for n in ("kv_map", "q_frames", "q_frame0")) and kw.get("kv_parts", 1) == 1 and kw.get("q_parts", 1) == 1
    q0, k0, v0 = _leaf(q), _leaf(k), _leaf(v)
    y = _tattn(q0, k0, v0, heads=heads, dh=dh, batch=batch, frames=frames, npix=npix, scale=dh ** -0.5 if scale is None else scale)
    return torch.autograd.grad(y, (q0, k0, v0), _d(dout)[:, :heads * dh])


def groupnorm_bwd(x, gamma, beta, dy, *, rows_per_group, eps, silu, groups=32):
    x0 = _leaf(x)
    y = _groupnorm(x0, _d(gamma), _d(beta), rows_per_group=rows_per_group, eps=eps, silu=silu, groups=groups)
    return torch.autograd.grad(y, x0, _d(dy))[0]


def layernorm_bwd(x, gamma, dy, *, eps=1e-5):
    x0 = _leaf(x)
    y = _layernorm(x0, _d(gamma), torch.zeros(x.shape[1], dtype=D), eps)
    return torch.autograd.grad(y, x0, _d(dy))[0]


def layernorm_bwd_params(x, dy, *, dgamma=None, dbeta=None, eps=1e-5):
    g0 = torch.ones(x.shape[1], dtype=D, requires_grad=True)
    b0 = torch.zeros(x.shape[1], dtype=D, requires_grad=True)
    dg, db = torch.autograd.grad(_layernorm(_d(x), g0, b0, eps), (g0, b0), _d(dy))
    if dgamma is not None:
        dgamma += dg
    if dbeta is not None:
        dbeta += db


def softmax_bwd_rows(P, dP, scale=1.0):
    """dS = P * (dP - sum_j P_j dP_j) * scale (me_softmax_bwd_rows; fp16 in, fp16 out on the device)."""
    p, dp = _d(P), _d(dP)
    return p * (dp - (p * dp).sum(dim=1, keepdim=True)) * scale


def relu_bwd(dy, out):
    return torch.where(_d(out) > 0, _d(dy), torch.zeros((), dtype=D))


def sumsq_absmax(x, out=None):
    """{sum x^2, max |x|}; a NaN anywhere makes both NaN, an inf (and no NaN) both +inf (include/motioned.h)."""
    xd = _d(x)
    m = xd.abs().max()
    if bool(torch.isnan(xd).any()):
        m = torch.tensor(math.nan, dtype=D)
    r = torch.stack([(xd * xd).sum(), m])
    if out is not None:
        out.copy_(r)
        return out
    return r


def adamw(p, m, v, g, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step, gnorm_sq=None, max_grad_norm=0.0, grad_scale=1.0):
    """torch.optim.AdamW's update written out element by element in fp64; clip_grad_norm_ folded in as me_adamw documents; a non-finite gnorm_sq: no-op.
    The hyper-parameters are the values me_adamw's ABI receives: fp32 (include/motioned.h), widened to fp64 here.  1 - float32(0.999) is 1.3e-5 away from
    0.001, which is a property of the signature and not an error of the kernel's arithmetic; the bias corrections travel as the fp32 of 1 - beta ** step."""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))    # noqa: E731
    bc1, bc2 = f32(1.0 - beta1 ** step), f32(1.0 - beta2 ** step)
    lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale = (f32(s) for s in (lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale))
    gs = grad_scale
    if gnorm_sq is not None:
        n2 = float(gnorm_sq.reshape(-1)[0])
        if not math.isfinite(n2):
            return
        gs *= min(1.0, max_grad_norm / (math.sqrt(n2) * grad_scale + 1e-6))
    gi = _d(g) * gs
    p *= 1.0 - lr * weight_decay
    m.copy_(beta1 * m + (1.0 - beta1) * gi)
    v.copy_(beta2 * v + (1.0 - beta2) * gi * gi)
    mhat, vhat = m / bc1, v / bc2
    p -= lr * mhat / (vhat.sqrt() + eps)


def cast_f16(dst, src):
    dst.copy_(src.detach().to(torch.float32).to(torch.float16))
    return dst


def cast_rows_f16(src, pad_cols):
    """fp16 [rows, pad_cols]: the columns of src cast, the padding zero (me_cast_rows_f16)."""
    out = torch.zeros((src.shape[0], pad_cols), dtype=torch.float16)
    out[:, :src.shape[1]] = src.detach().to(torch.float32).to(torch.float16)
    return out


def mse_seed(eps_u, target, *, eps_c=None, x=None, guidance=1.0, ca=0.0, cb=1.0, coef=1.0):
    nb, C, f, h, w = target.shape
    to5 = lambda r: _d(r)[:, :C].reshape(nb, f, h * w, C).permute(0, 3, 1, 2).reshape(nb, C, f, h, w)   # noqa: E731
    e = to5(eps_u)
    if eps_c is not None:
        e = e + guidance * (to5(eps_c) - e)
    rec = cb * e + (ca * _d(x) if x is not None else 0.0)
    diff = rec - _d(target)
    return diff, (coef * diff).permute(0, 2, 3, 4, 1).reshape(-1, C).contiguous()
