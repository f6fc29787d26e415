"""What the one-call 3x3 weight gradient (me_conv_dw, csrc/tune.hip) costs at the UNet's convolutions of the stage-1 training size (8 frames x 64^2 latents),
against the only form the dense kernel offers: NINE me_gemm_dw launches at the same M, N, K (the same number of products, dY read nine times; it cannot do
the 3x3 gather, so it multiplies un-gathered rows -- a yardstick for time, not for values).

    python tools/conv_dw_bench.py [--warmup 5 --rounds 7 --calls 10] [--out profiles/conv_dw_bench.json]

In ONE process, per shape: `warmup` calls of each side, then `rounds` alternations of (`calls` x me_conv_dw, `calls` x nine me_gemm_dw), each window timed by a
pair of stream events; the medians over the rounds are reported as ms per weight gradient with TFLOP/s = 2 * 9 * M * N * K / time beside them.  Required:
me_conv_dw's median is not above the yardstick's on any shape (`ok`); a shape that misses is reported, with the kernel's resource usage.  One JSON line on
stdout; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# conv_dw_kernel as hipcc -Rpass-analysis=kernel-resource-usage reports it for gfx950 (both dY instantiations)
RESOURCES = {"vgprs": 64, "agprs": 144, "scratch_bytes_per_lane": 0, "lds_bytes_per_block": 51200, "waves_per_simd": 2, "block": 256, "tile": "64 k x 64 n x 9 taps x 32 rows"}

# name, images, Hin, Win, N, K, stride, ups   (8 frames; level l has (64 >> l)^2 pixels)
SHAPES = [
    ("level0 32768x320x320", 8, 64, 64, 320, 320, 1, 0),
    ("level1 8192x640x640", 8, 32, 32, 640, 640, 1, 0),
    ("level2 2048x1280x1280", 8, 16, 16, 1280, 1280, 1, 0),
    ("level3 512x1280x1280", 8, 8, 8, 1280, 1280, 1, 0),
    ("downsampler level0 stride 2 -> 8192x320x320", 8, 64, 64, 320, 320, 2, 0),
    ("downsampler level1 stride 2 -> 2048x640x640", 8, 32, 32, 640, 640, 2, 0),
    ("upsampler to level0 ups -> 32768x640x640", 8, 32, 32, 640, 640, 1, 1),
    ("upsampler to level1 ups -> 8192x1280x1280", 8, 16, 16, 1280, 1280, 1, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_dw_bench: needs a GPU (a timing taken anywhere else says nothing)")
    from motioneditor_amd import capi, ops

    def timed(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / count

    rows = []
    for name, n_img, Hin, Win, N, K, stride, ups in SHAPES:
        Hout, Wout = ((Hin << ups) - 1) // stride + 1, ((Win << ups) - 1) // stride + 1
        M = n_img * Hout * Wout
        g = torch.Generator().manual_seed(N + K + M)
        x = (torch.randn(n_img * Hin * Win, K, generator=g) * 0.5).half().cuda()
        xd = (torch.randn(M, K, generator=g) * 0.5).half().cuda()            # the dense yardstick reads M un-gathered rows
        dy = (torch.randn(M, N, generator=g) * 0.5).half().cuda()             # fp16 dY, as the tape hands it to both kernels' MFMAs after the cast
        d9, d1 = torch.zeros(N, 9, K, device="cuda"), torch.zeros(N, 1, K, device="cuda")
        conv = lambda: ops.gemm_dw(dy, x, dst=d9, taps=9, K=K, M=M, conv=(Hin, Win, Hout, Wout, stride, ups))   # noqa: E731

        def dense9():
            for _ in range(9):
                ops.gemm_dw(dy, xd, dst=d1, taps=1, K=K, M=M)
        for _ in range(a.warmup):
            conv()
            dense9()
        torch.cuda.synchronize()
        tc, td = [], []
        for _ in range(a.rounds):
            tc.append(timed(conv, a.calls))
            td.append(timed(dense9, a.calls))
        mc, md = statistics.median(tc), statistics.median(td)
        flop = 2.0 * 9 * M * N * K
        row = {"shape": name, "M": M, "N": N, "K": K, "stride": stride, "ups": ups, "splits": int(capi.lib().me_conv_dw_splits(M, N, K)),
               "conv_dw_ms": round(mc, 4), "nine_gemm_dw_ms": round(md, 4), "conv_dw_tflops": round(flop / mc / 1e9, 1), "nine_gemm_dw_tflops": round(flop / md / 1e9, 1),
               "conv_dw_ms_min_max": [round(min(tc), 4), round(max(tc), 4)], "nine_gemm_dw_ms_min_max": [round(min(td), 4), round(max(td), 4)],
               "ratio": round(mc / md, 3), "ok": mc <= md}
        if not row["ok"]:
            row["resources"] = RESOURCES
        rows.append(row)
        print(f"{name}: me_conv_dw {mc:.3f} ms ({row['conv_dw_tflops']} TFLOP/s), nine me_gemm_dw {md:.3f} ms ({row['nine_gemm_dw_tflops']} TFLOP/s), ratio {row['ratio']}",
              file=sys.stderr, flush=True)
    res = {"tool": "conv_dw_bench", "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds, "calls": a.calls, "dy": "fp16",
           "resources": RESOURCES, "all_ok": all(r["ok"] for r in rows), "shapes": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
