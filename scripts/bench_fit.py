"""fit_channels end to end: Model.run_u8 of one 1080p frame through 4x RRDBNet-23 (synthetic weights, fp16, chop path) as BGR, as BGRA with an
opaque alpha plane and as BGRA with a varying one -- the same pixels.  The frame lives on the GPU (no PCIe in the timing); every step is one
run_u8 with a device synchronisation after it.  The three kinds are interleaved round by round and the median per kind is printed, one JSON line
each, with the shader clock rocm-smi reports after the run.

    python scripts/bench_fit.py [--steps 5] [--warmup 2]

Kernel times: run it under `rocprofv3 --kernel-trace --stats` (a run of its own) and compare the FIT instantiations of k_extract_u8 /
k_recompose_u8 with those of the BGR frame, or run `scripts/bench_seamless.py --kernels-only`."""
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

    from innfer_amd import run as R, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=23, scale=4), 0).items()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "4x_rrdb23.pth")
        torch.save(sd, path)
        m = R.Model(path, "infer", 4, device=dev)
    bgra = synth.image_u8(a.height, a.width, 4, 1)
    opaque = bgra.copy()
    opaque[:, :, 3] = 255
    kinds = {"bgr": (np.ascontiguousarray(bgra[:, :, :3]), False), "bgra_opaque": (opaque, True), "bgra_alpha": (bgra, True)}
    imgs = {k: (torch.from_numpy(im).to(dev), fit) for k, (im, fit) in kinds.items()}
    outs = {k: torch.empty((a.height * 4, a.width * 4, im.shape[2]), dtype=torch.uint8, device=dev) for k, (im, _) in imgs.items()}
    times = {k: [] for k in imgs}
    for step in range(a.warmup + a.steps):
        for k, (im, fit) in imgs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            m.run_u8(im, out=outs[k], fit_channels=fit)
            torch.cuda.synchronize(dev)
            if step >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    clk = sclk_mhz()
    base = float(np.median(times["bgr"]))
    for k, ts in times.items():
        med = float(np.median(ts))
        print(json.dumps({"kind": k, "frame": f"{a.width}x{a.height}", "model": "4x RRDBNet-23 fp16 chop", "ms_median": round(med, 2),
                          "ms_min": round(min(ts), 2), "vs_bgr": round(med / base, 3), "steps": a.steps, "sclk_mhz": clk}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
