"""The colour fixes on the MI355X (measurement only; needs the GPU).

(a) kernels: innfer_color_fix_mode of the three modes on device buffers, 1080 x 1920 -> 4320 x 7680, C = 3 by default.  Every round times each mode once
    (device events around `--calls` back-to-back calls), so the modes alternate; medians over the rounds and the round-to-round spread (max / min).  For
    wavelet and adain the achieved GB/s of ALGORITHMIC bytes: LR read + SR read + SR written, plus one more SR read for adain's reduction.
(b) host image -> host image: Model.run_u8(img, color_fix='lowfreq') -- one upload, the network, the fix, one download -- against the two separate calls
    run_u8(img) and utils.color_fix(img, sr) (what the command line did before: the SR image crosses PCIe three times), with a compact model, at
    270 x 480 -> 1080 x 1920 and 1080 x 1920 -> 4320 x 7680.  Alternating, host clock around calls that end in the download; medians, the spread of the
    separate calls' own rounds, and a check that both returned the same bytes.
The shader clock is read (rocm-smi, read only) after the runs.

    python scripts/time_colorfix.py [--rounds 10] [--calls 5] [--sizes 270x480 1080x1920] [--skip-model] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from innfer_amd import lib as L, synth                  # noqa: E402
from innfer_amd.utils import utils as U                 # noqa: E402
from time_batch import shader_clock_mhz                 # noqa: E402


def kernels(h, w, s, C, rounds, calls):
    dev = torch.device("cuda:0")
    a = torch.from_numpy(synth.image_u8(h, w, C, 1)).to(dev)
    b = torch.from_numpy(synth.image_u8(h * s, w * s, C, 2)).to(dev)
    out = torch.empty_like(b)
    stream = torch.cuda.current_stream().cuda_stream
    ws = {m: torch.empty(max(1, L.lib.innfer_color_fix_mode_workspace_bytes(code, h, w, h * s, w * s, C)), dtype=torch.uint8, device=dev)
          for m, code in L.COLOR_FIX_MODES.items()}

    def call(m):
        L.check(L.lib.innfer_color_fix_mode(L.COLOR_FIX_MODES[m], a.data_ptr(), h, w, b.data_ptr(), h * s, w * s, C, out.data_ptr(), ws[m].data_ptr(),
                                            ws[m].numel(), stream))
    ms = {m: [] for m in L.COLOR_FIX_MODES}
    for r in range(rounds + 2):                                             # two rounds of warm-up
        for m in ms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call(m)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ms[m].append(e0.elapsed_time(e1) / calls)
    nbytes = {"wavelet": a.numel() + 2 * b.numel(), "adain": a.numel() + 3 * b.numel()}
    res = {"lr": [h, w], "sr": [h * s, w * s], "C": C, "rounds": rounds, "calls_per_round": calls, "workspace_bytes": {m: int(L.lib.innfer_color_fix_mode_workspace_bytes(code, h, w, h * s, w * s, C)) for m, code in L.COLOR_FIX_MODES.items()}}
    for m, v in ms.items():
        med = statistics.median(v)
        res[m] = {"ms": round(med, 4), "spread_max_over_min": round(max(v) / min(v), 3)}
        if m in nbytes:
            res[m]["algorithmic_GB_per_s"] = round(nbytes[m] / med / 1e6, 1)
    return res


def host_to_host(sizes, rounds):
    import _compact_ref as CR
    from innfer_amd.run import Model
    m = Model(None, "infer", None, state_dict=CR.fill(3, 64, 16, 4, seed=16))
    res = {"model": "SRVGGNetCompact num_conv 16, 4x, synth weights, fp16", "sizes": {}}
    for h, w in sizes:
        img = synth.image_u8(h, w, 3, 9)
        runs = {"separate": lambda: U.color_fix(img, m.run_u8(img)), "fused": lambda: m.run_u8(img, color_fix="lowfreq")}
        sec = {k: [] for k in runs}
        same = None
        for r in range(rounds + 2):
            got = {}
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[k] = fn()
                torch.cuda.synchronize()
                if r >= 2:
                    sec[k].append(time.perf_counter() - t0)
            if same is None:
                same = bool(np.array_equal(got["separate"], got["fused"]))
        med = {k: statistics.median(v) for k, v in sec.items()}
        res["sizes"][f"{h}x{w}"] = {"same_bytes": same, "separate_ms": round(med["separate"] * 1e3, 3), "fused_ms": round(med["fused"] * 1e3, 3),
                                    "separate_spread_max_over_min": round(max(sec["separate"]) / min(sec["separate"]), 3),
                                    "fused_spread_max_over_min": round(max(sec["fused"]) / min(sec["fused"]), 3),
                                    "fused_over_separate": round(med["fused"] / med["separate"], 3)}
        print(f"{h}x{w}", json.dumps(res["sizes"][f"{h}x{w}"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--lr", default="1080x1920")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=["270x480", "1080x1920"])
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    h, w = (int(v) for v in args.lr.split("x"))
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = kernels(h, w, args.scale, args.channels, args.rounds, args.calls)
    print("kernels", json.dumps(res["kernels"]), flush=True)
    if not args.skip_model:
        res["host_to_host"] = host_to_host([tuple(int(v) for v in s.split("x")) for s in args.sizes], args.rounds)
    res["sclk_mhz_after"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
