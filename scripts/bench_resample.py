"""`-outscale` kernel alone and end to end: a 1080p BGR frame through the 4x RRDBNet-23 (synthetic weights, fp16, chop path) with outscale=2 --

    kernel     innfer_resample_inthwc alone, 4320 x 7680 x 3 -> 2160 x 3840 (lanczos; --all-filters: every filter), device events around `--reps`
               launches, median of `--steps` windows; the rate is the algorithm's bytes (source read once + result written once) over that time
    plain      run_u8(img)                                        (numpy in, numpy out: upload, forward, the 100 MB download)
    outscale   run_u8(img, outscale=2)                            (upload, forward, resample on the device, the 25 MB download)
    host       PIL resize(LANCZOS) of run_u8(img)                  (what a user has today: the full download, then a host resize; left out where
               PIL is absent)

The end-to-end forms are interleaved round by round; medians, one JSON line per form.  Nothing here is a gate.

    python scripts/bench_resample.py [--steps 5] [--warmup 2] [--reps 20] [--kernel-only] [--all-filters]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def sclk_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
    except Exception:
        return None
    m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", out)
    return int(m.group(1)) if m else None


def main(argv=None):
    import tempfile

    import numpy as np
    import torch

    from innfer_amd import lib as L, run as R, synth
    from innfer_amd.utils import utils as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nb", type=int, default=23)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--all-filters", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    s, F = 4, 2
    h, w, C = 1080, 1920, 3
    H, W, oh, ow = h * s, w * s, h * F, w * F

    # ---- the kernel alone
    src = torch.from_numpy(synth.image_u8(H, W, C, 1)).to(dev)
    dst = torch.empty((oh, ow, C), dtype=torch.uint8, device=dev)
    for name in (U.RESAMPLE_FILTERS if a.all_filters else ("lanczos",)):
        fn = lambda: U.resample(src, size=(oh, ow), filter=name, out=dst)        # plans cached after the first call
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / a.reps)
        ms = float(np.median(ts[a.warmup:]))
        Th, Tv = L.resample_taps(W, ow, name), L.resample_taps(H, oh, name)
        print(json.dumps({"kernel": "innfer_resample_inthwc", "filter": name, "shape": f"{H}x{W}x{C} -> {oh}x{ow}", "taps": [Th, Tv],
                          "fused": L.lib.innfer_resample_workspace_bytes(H, W, C, oh, ow, Th, Tv) == 0, "ms": round(ms, 4),
                          "GBps": round((src.numel() + dst.numel()) / ms / 1e6, 1), "reps": a.reps, "sclk_mhz": sclk_mhz()}), flush=True)
    del src, dst
    if a.kernel_only:
        return 0

    # ---- end to end
    try:
        from PIL import Image
    except ImportError:
        Image = None
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=a.nb, scale=s), 0).items()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "4x_rrdb.pth")
        torch.save(sd, path)
        m = R.Model(path, "infer", s, device=dev)
    img = synth.image_u8(h, w, C, 2)
    forms = {"plain": lambda: m.run_u8(img), "outscale": lambda: m.run_u8(img, outscale=F)}
    if Image is not None:
        forms["host"] = lambda: np.asarray(Image.fromarray(m.run_u8(img)).resize((ow, oh), Image.LANCZOS))
    times = {k: [] for k in forms}
    for step in range(a.warmup + a.steps):
        for k, fn in forms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if step >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    for form, ts in times.items():
        med = float(np.median(ts))
        print(json.dumps({"image": f"frame {w}x{h} BGR", "form": form, "model": f"4x RRDBNet-{a.nb} fp16 chop", "result": f"{H}x{W}" if form == "plain" else f"{oh}x{ow}",
                          "ms_median": round(med, 2), "ms_min": round(min(ts), 2), "vs_plain": round(med / float(np.median(times["plain"])), 3),
                          "steps": a.steps, "sclk_mhz": sclk_mhz()}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
