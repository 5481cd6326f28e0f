"""The kernels of a DAT block on the MI355X, each launch alone (measurement only; needs the GPU).  Whole forwards are not timed here yet.

Three published block shapes (as recalled from the DAT release; random data, fp16 slabs):
    DAT        embed_dim 180, 6 heads, split [8, 32], expansion_factor 4      (the feed-forward's half: 360 channels, a slab of 384)
    DAT-S      embed_dim 180, 6 heads, split [8, 16], expansion_factor 2      (180 channels, a slab of 192)
    DAT-light  embed_dim 60,  6 heads, split [8, 32], expansion_factor 2      (60 channels, a slab of 64)
each on 16 tiles of 200 x 200 (what the chop path hands an engine) and on 540 x 960 whole.  Per shape, alternating round after round, the library's launch timer
(innfer_timer_start / innfer_timer_stop: a device-event pair around every launch) around
    the rectangular window attention, not shifted and shifted            (innfer_window_attention_rect)
    the channel attention's Gram + norms, its merge / softmax, its apply  (innfer_channel_attention_scores: two launches; innfer_channel_attention_apply)
    the depthwise 3 x 3 with GELU on embed_dim channels, and times a gate on the feed-forward's half      (innfer_dwconv3x3, epilogues 1 and 2)
    the pool + GELU excite and the interaction mix                        (innfer_chan_attn_excite_gelu: two launches; innfer_aim_mix)
    LayerNorm over the feed-forward's half                                (innfer_layer_norm_wide)
Medians and minima over the rounds, with the algorithmic GB/s and TFLOP/s the launch timer's own byte and flop counts give.  The shader clock is read after the runs.

    python scripts/time_dat.py [--rounds 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402

MODELS = {"DAT": (180, 6, 32, 4.0), "DAT-S": (180, 6, 16, 2.0), "DAT-light": (60, 6, 32, 2.0)}
SHAPES = {"16x200x200": (16, 200, 200), "1x540x960": (1, 540, 960)}


def launches(dev, model, shape):
    """{name: callable} of the single launches of one block shape on one grid; every buffer is allocated here, once."""
    Cc, nH, s1, ef = MODELS[model]
    N, H, W = SHAPES[shape]
    d, cp, half = Cc // nH, -(-Cc // 64) * 64, int(Cc * ef) // 2
    hp, T, HW = -(-half // 64) * 64, 8 * s1, H * W
    G = N * HW * 32
    rnd = lambda groups: (torch.rand((groups, G), device=dev) * 2 - 1).half()          # (random data: zeros would read fast)
    qkv = rnd(3 * nH)
    qkv.view(3 * nH, -1, 32)[:, :, d:] = 0
    att = torch.empty((nH, G), dtype=torch.float16, device=dev)
    xa, xb, xo = rnd(cp // 32), rnd(cp // 32), torch.empty((cp // 32, G), dtype=torch.float16, device=dev)
    ha, hb, ho = rnd(hp // 32), rnd(hp // 32), torch.empty((hp // 32, G), dtype=torch.float16, device=dev)
    table = np.ascontiguousarray(synth.uniform((nH, T, T), 3, -2, 2))
    temp = np.ascontiguousarray(synth.uniform((nH,), 4, 0.5, 2.0))
    A = torch.empty(N * nH * 1024, dtype=torch.float32, device=dev)
    wb = L.lib.innfer_channel_attention_work_bytes(N, HW, nH)
    work = torch.empty(wb // 4, dtype=torch.float32, device=dev)
    pb = L.lib.innfer_chan_attn_work_bytes(N, HW, cp)
    pool = torch.empty(pb // 4, dtype=torch.float32, device=dev)
    gate = torch.empty(N * cp, dtype=torch.float32, device=dev)
    f = lambda shp, seed, lo=-1.0, hi=1.0: np.ascontiguousarray(synth.uniform(shp, seed, lo, hi))
    taps_c, bias_c, taps_h, bias_h = f((Cc, 9), 5), f((Cc,), 6), f((half, 9), 7), f((half,), 8)
    hc, hs = Cc // 8, Cc // 16
    cw1, cb1, cw2, cb2 = f((hc, Cc), 9), f((hc,), 10), f((Cc, hc), 11), f((Cc,), 12)
    sw1, sb1, sw2 = f((hs, Cc), 13), f((hs,), 14), f((hs,), 15)
    gam, bet = f((half,), 16, 0.5, 1.5), f((half,), 17)
    p = lambda a: a.ctypes.data
    lib = L.lib
    return {
        "rect attention": lambda: L.check(lib.innfer_window_attention_rect(qkv.data_ptr(), G, att.data_ptr(), G, p(table), N, H, W, nH, d, 8, s1, 0, None)),
        "rect attention, shifted": lambda: L.check(lib.innfer_window_attention_rect(qkv.data_ptr(), G, att.data_ptr(), G, p(table), N, H, W, nH, d, 8, s1, 1, None)),
        "channel attention scores": lambda: L.check(lib.innfer_channel_attention_scores(qkv.data_ptr(), G, N, HW, nH, d, p(temp), A.data_ptr(), None, work.data_ptr(), wb, None)),
        "channel attention apply": lambda: L.check(lib.innfer_channel_attention_apply(qkv.data_ptr(), G, att.data_ptr(), G, A.data_ptr(), N, HW, nH, d, None)),
        "dwconv + GELU (C)": lambda: L.check(lib.innfer_dwconv3x3(xa.data_ptr(), G, None, 0, xo.data_ptr(), G, N, H, W, Cc, cp, p(taps_c), p(bias_c), 1, None)),
        "dwconv x gate (hidden / 2)": lambda: L.check(lib.innfer_dwconv3x3(ha.data_ptr(), G, hb.data_ptr(), G, ho.data_ptr(), G, N, H, W, half, hp, p(taps_h), p(bias_h), 2, None)),
        "pool + GELU excite": lambda: L.check(lib.innfer_chan_attn_excite_gelu(xa.data_ptr(), G, N, HW, Cc, cp, hc, p(cw1), p(cb1), p(cw2), p(cb2), gate.data_ptr(), None,
                                                                               pool.data_ptr(), pb, None)),
        "interaction mix": lambda: L.check(lib.innfer_aim_mix(xa.data_ptr(), G, xb.data_ptr(), G, xo.data_ptr(), G, gate.data_ptr(), N, HW, Cc, cp, hs, p(sw1), p(sb1), p(sw2),
                                                              0.0, None)),
        "layer norm (hidden / 2)": lambda: L.check(lib.innfer_layer_norm_wide(ha.data_ptr(), G, ho.data_ptr(), G, N * HW, half, hp, p(gam), p(bet), 1e-5, None)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    for model in MODELS:
        for shape in SHAPES:
            fns = launches(dev, model, shape)
            runs = {k: [] for k in fns}
            for r in range(args.rounds + 2):
                for k, fn in fns.items():
                    t = L.timed_launches(fn)
                    if r >= 2:
                        runs[k].append(t)
            out = {}
            for k, v in runs.items():
                for i in range(len(v[0])):          # (a call that makes two launches reports each)
                    ms = [t[i][1] for t in v]
                    med = statistics.median(ms)
                    out[f"{k}: {v[0][i][0]}"] = dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), gbytes_per_s=round(v[0][i][3] / med / 1e6, 1),
                                                     tflops_per_s=round(v[0][i][2] / med / 1e9, 2))
            res[f"{model} {shape}"] = out
            del fns
            torch.cuda.empty_cache()
    res["sclk_mhz_after"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
