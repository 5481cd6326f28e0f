#!/usr/bin/env python3
"""Cost of the folded pixel_unshuffle: the 2x BasicSR RRDBNet-23 on a 1080p frame against today's 4x RRDBNet-23 on the frame of its LR grid.

  (a) RealESRGANNet(scale=2, num_block=23) on 1x3x1080x1920 fp16   -- first conv: conv_first_unshuffle.hip (12 channels, 6x6 window, stride 2)
  (b) RRDBNet(nb=23, upscale=4)            on 1x3x540x960   fp16   -- first conv: conv_first.hip; the same trunk and tail on the same 540 x 960 grid
  (c) the first-conv line of innfer_net_forward_timed for both (median of the per-launch event times)

(a) and (b) run in one process, alternating, after warm-up; each timed window is `--reps` forwards between two device events.  (a) - (b) should be the
first convs' difference.  Also reports (c) for the 1x form (48 channels, 12x12 window) on its own.  Prints one JSON line.

    python scripts/time_realesrgan.py [--reps 10] [--rounds 7]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from innfer_amd import lib as L, synth  # noqa: E402
from innfer_amd.architectures.RRDBNet_arch import RealESRGANNet, RRDBNet  # noqa: E402
from innfer_amd.architectures.keys import realesrgan_shapes, rrdbnet_shapes  # noqa: E402


def load(net, shapes, seed):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}, strict=True)
    return net.cuda().eval()


def window(net, x, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        net(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def first_conv_ms(net, x, n=15):
    """median time of launch 0 (kind 0: the first conv) over n timed forwards."""
    net(x)
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    (hh, ww), _ = net._io_sizes(H, W, s)
    out = torch.empty((N, net.out_nc, hh, ww), dtype=x.dtype, device=x.device)
    cap = 4096
    ms, fl, by, kind, nl = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int * cap)(), C.c_int()
    got = []
    for _ in range(n):
        L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, net._ws.data_ptr(), net._ws.numel(),
                                               torch.cuda.current_stream().cuda_stream, cap, ms, fl, by, kind, C.byref(nl)))
        assert kind[0] == 0
        got.append(ms[0])
    return statistics.median(got), by[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nb", type=int, default=23)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    nb = a.nb
    net2 = load(RealESRGANNet(3, 3, 2, 64, nb, 32), realesrgan_shapes(3, 3, 2, 64, nb, 32), 1)
    net4 = load(RRDBNet(3, 3, 64, nb, upscale=4), rrdbnet_shapes(nb=nb, scale=4), 2)
    net1 = load(RealESRGANNet(3, 3, 1, 64, nb, 32), realesrgan_shapes(3, 3, 1, 64, nb, 32), 3)
    xa = torch.from_numpy(synth.uniform((1, 3, 1080, 1920), 5)).cuda().half()
    xb = torch.from_numpy(synth.uniform((1, 3, 540, 960), 6)).cuda().half()
    for _ in range(3):
        net2(xa); net4(xb)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(window(net2, xa, a.reps))
        tb.append(window(net4, xb, a.reps))
    fa, ba = first_conv_ms(net2, xa)
    fb, bb = first_conv_ms(net4, xb)
    f1, b1 = first_conv_ms(net1, xa)
    med = statistics.median
    print(json.dumps({
        "a_2x_1080p_ms": round(med(ta), 4), "a_spread_ms": [round(min(ta), 4), round(max(ta), 4)],
        "b_4x_540p_ms": round(med(tb), 4), "b_spread_ms": [round(min(tb), 4), round(max(tb), 4)],
        "a_minus_b_ms": round(med(ta) - med(tb), 4),
        "c_first_conv_unshuffle2_ms": round(fa, 4), "c_first_conv_unshuffle2_GBps": round(ba / fa / 1e6, 1),
        "c_first_conv_plain_ms": round(fb, 4), "c_first_conv_plain_GBps": round(bb / fb / 1e6, 1),
        "first_conv_unshuffle4_1080p_ms": round(f1, 4), "first_conv_unshuffle4_GBps": round(b1 / f1 / 1e6, 1),
        "nb": nb, "reps": a.reps, "rounds": a.rounds}))


if __name__ == "__main__":
    main()
