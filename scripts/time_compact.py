"""SRVGGNetCompact on the MI355X: what the act-8 epilogue costs a launch, and whole 1080p frames (measurement only; needs the GPU).

(a) one 64 -> 64 conv at 1 x 64 x 1080 x 1920 (plane-order panels, as the networks run it) with act 8 (per-channel slopes) against the same launch with act 1
    (LeakyReLU(0.2)): the two alternate in one process, device-event time per launch (the library's launch timer), median and minimum of the rounds.
(b) innfer_net_forward_timed of whole 1080p frames, num_conv 16 and 32, scale 4, fp16 and uint8 I/O: per-kernel times of the median frame, summed by kind
    (0 first conv, 64 / 32 the slab convs, 6000 the shuffle-add tail), and the frame's host-clock time around a synchronised forward.

    python scripts/time_compact.py [--rounds 30] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import _compact_ref as CR           # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402


def one_launch(dev, rounds):
    N, Cc, K, H, W = 1, 64, 64, 1080, 1920
    G = N * H * W * 32
    x = (torch.rand((2, G), device=dev) * 2 - 1).half()               # (random data: zeros would read fast)
    w = np.ascontiguousarray(synth.uniform((K, Cc, 3, 3), 2, -1, 1) / np.float32(np.sqrt(9 * Cc)))
    packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(K, Cc), np.uint8)
    L.check(L.lib.innfer_pack_conv3x3_rows(w.ctypes.data, K, Cc, 1, packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    d_bias = torch.from_numpy(synth.uniform((64,), 3, -1, 1)).to(dev)
    d_slope = torch.from_numpy(synth.uniform((64,), 4, -0.25, 0.75)).to(dev)
    out = torch.empty((2, G), dtype=torch.float16, device=dev)
    a = L.ConvArgs(d_in=x.data_ptr(), in_group_stride=G, C=Cc, d_packed=d_packed.data_ptr(), d_bias=d_bias.data_ptr(), d_out=out.data_ptr(), out_group_stride=G,
                   K=K, N=N, H=H, W=W, plane_rows=1)

    def run(act):
        a.act = act
        if act == 8:
            L.check(L.lib.innfer_conv3x3_f16_slope(C.byref(a), d_slope.data_ptr(), None))
        else:
            L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))

    for _ in range(5):
        run(1); run(8)
    torch.cuda.synchronize()
    ms = {1: [], 8: []}
    for _ in range(rounds):
        for act in (1, 8):
            ms[act].append(L.timed_launches(lambda: run(act))[0][1])
    flops = 2.0 * 9 * K * Cc * N * H * W
    return {f"act{act}": dict(median_ms=statistics.median(v), min_ms=min(v), tflops_median=flops / statistics.median(v) / 1e9) for act, v in ms.items()}


def shader_clock_mhz():
    """The shader clock rocm-smi shows right after the timed work (read only), or None."""
    import re
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def frames(dev, num_conv, u8, rounds):
    from innfer_amd.architectures.SRVGG_arch import SRVGGNetCompact
    net = SRVGGNetCompact(3, 3, 64, num_conv, 4)
    net.load_state_dict(CR.fill(3, 64, num_conv, 4, seed=num_conv), strict=True)
    net = net.to(dev).eval()
    H, W = 1080, 1920
    if u8:
        x = torch.from_numpy(synth.image_u8(H, W, 3, 1)).to(dev)
        y = net.forward_u8(x)
        dt = L.U8
    else:
        x = torch.from_numpy(synth.uniform((1, 3, H, W), 5)).half().to(dev)
        y = net(x)
        dt = L.F16
    ws, stream = net._ws, torch.cuda.current_stream(dev).cuda_stream
    cap = 256
    ms, fl, by, kind, n = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int * cap)(), C.c_int()
    per, wall = [], []
    for r in range(rounds + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), dt, y.data_ptr(), dt, 1, H, W, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), dt, y.data_ptr(), dt, 1, H, W, ws.data_ptr(), ws.numel(), stream, cap, ms, fl, by, kind, C.byref(n)))
        if r >= 3:
            wall.append((t1 - t0) * 1e3)
            per.append([(kind[i], ms[i]) for i in range(n.value)])
    sums = sorted(sum(m for _, m in p) for p in per)
    med = per[[sum(m for _, m in p) for p in per].index(sums[len(sums) // 2])]
    by_kind = {}
    for k, m in med:
        e = by_kind.setdefault(str(k), [0, 0.0]); e[0] += 1; e[1] += m
    layer = [m for k, m in med if k == 64]
    return dict(num_conv=num_conv, io="uint8" if u8 else "fp16", launches=len(med), kernel_sum_ms_median=sums[len(sums) // 2], kernel_sum_ms_min=sums[0],
                frame_wall_ms_median=statistics.median(wall), frame_wall_ms_min=min(wall), by_kind={k: dict(launches=c, ms=m) for k, (c, m) in by_kind.items()},
                ms_per_64_output_layer=(sum(layer) / len(layer)) if layer else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "one_launch_1x64x1080x1920": one_launch(dev, args.rounds)}
    res["sclk_mhz_after_launches"] = shader_clock_mhz()
    res["frames_1080p_x4"] = []
    for nc in (16, 32):
        for u8 in (False, True):
            res["frames_1080p_x4"].append(frames(dev, nc, u8, max(5, args.rounds // 3)))
    res["sclk_mhz_after_frames"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
