"""fp64 references of the folded nearest-2x convolution (me_gemm gather mode ups = 3), written from its definition and shared by
tests/test_ups_fold_cpu.py and tests/test_ups_fold_gpu.py.  Plain helpers, CPU torch only.

Activations are rows [(img, y, x), C] (channels-last); weights are [N, 9, K] (tap = 3 ky + kx) or folded [N, 16, K] (index 4 (2 py + px) + 2 ty + tx:
tap (ty, tx) of output parity (py, px) reads low-res pixel (y + py - 1 + ty, x + px - 1 + tx), zero outside the image)."""
import torch
import torch.nn.functional as F


def rows_to_nchw(x: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    return x.double().reshape(n_img, H, W, -1).permute(0, 3, 1, 2)


def nchw_to_rows(y: torch.Tensor) -> torch.Tensor:
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def conv_ups_ref(x: torch.Tensor, w9: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    """conv2d(interpolate(x, 2, 'nearest'), W, padding = 1) in fp64: rows [n_img * 2H * 2W, N]."""
    n, _, k = w9.shape
    w = w9.double().reshape(n, 3, 3, k).permute(0, 3, 1, 2)
    up = F.interpolate(rows_to_nchw(x, n_img, H, W), scale_factor=2, mode="nearest")
    return nchw_to_rows(F.conv2d(up, w, padding=1))


def conv_fold_ref(x: torch.Tensor, w16: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    """The four 2x2-tap convolutions in fp64, straight from the definition of the 16-tap layout: rows [n_img * 2H * 2W, N]."""
    n = w16.shape[0]
    xp = F.pad(rows_to_nchw(x, n_img, H, W), (1, 1, 1, 1))       # padded pixel (y + 1, x + 1) = pixel (y, x)
    out = torch.zeros((n_img, n, 2 * H, 2 * W), dtype=torch.float64)
    w16 = w16.double()
    for py in range(2):
        for px in range(2):
            acc = torch.zeros((n_img, n, H, W), dtype=torch.float64)
            for ty in range(2):
                for tx in range(2):
                    src = xp[:, :, py + ty:py + ty + H, px + tx:px + tx + W]
                    acc += torch.einsum("bchw,nc->bnhw", src, w16[:, 4 * (2 * py + px) + 2 * ty + tx])
            out[:, :, py::2, px::2] = acc
    return nchw_to_rows(out)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
