"""Model.run_u8_batch against the per-image run_u8 loop on the MI355X (measurement only; needs the GPU).

Host numpy images through one model in ONE process: every round runs the loop `[m.run_u8(im) for im in imgs]` -- the code as it was, so the baseline --
and then `m.run_u8_batch` over consecutive chunks of B images for every B, host clock around each pass (both end in the download of the last result, so
nothing is in flight when the clock stops).  Medians of images/s over the rounds, the speed-up over the loop, the round-to-round spread of the loop
(max / min), and a check that the two paths returned the same bytes.  The shader clock is read (rocm-smi, read only) after each model.

    python scripts/time_batch.py [--nets rrdb compact] [--sets 64 128 256 512 mixed] [--images 64] [--batches 1 4 16 64] [--rounds 10] [--out FILE]
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

import _compact_ref as CR           # noqa: E402
from innfer_amd import synth        # noqa: E402
from innfer_amd.run import Model    # noqa: E402


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


def model(net):
    if net == "rrdb":
        sd = synth.fill_state_dict(synth.rrdbnet_shapes(nb=23, scale=4), 0)
        return Model(None, "infer", 4, state_dict={k: torch.from_numpy(v) for k, v in sd.items()}), "RRDBNet nb 23, 4x, synth weights, fp16"
    return Model(None, "infer", None, state_dict=CR.fill(3, 64, 16, 4, seed=16)), "SRVGGNetCompact num_conv 16, 4x, synth weights, fp16"


def image_set(name, n):
    if name == "mixed":                                                 # 256 .. 700 px per side, seeded
        rng = np.random.RandomState(5)
        sizes = [(int(rng.randint(256, 701)), int(rng.randint(256, 701))) for _ in range(n)]
    else:
        sizes = [(int(name), int(name))] * n
    return [synth.image_u8(h, w, 3, 100 + i) for i, (h, w) in enumerate(sizes)]


def chunks(m, imgs, B):
    out = []
    for i in range(0, len(imgs), B):
        out += m.run_u8_batch(imgs[i:i + B])
    return out


def measure(m, imgs, batches, rounds):
    runs = {"loop": lambda: [m.run_u8(im) for im in imgs]}
    runs.update({f"batch_{B}": (lambda B=B: chunks(m, imgs, B)) for B in batches})
    sec = {k: [] for k in runs}
    same = True
    for r in range(rounds + 2):                                         # two rounds of warm-up (workspaces, the allocator's blocks, pinned buffers)
        ref = None
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r >= 2:
                sec[k].append(dt)
            if r == 0:
                if ref is None:
                    ref = res
                else:
                    same = same and all(np.array_equal(a, b) for a, b in zip(ref, res))
    n = len(imgs)
    loop = statistics.median(sec["loop"])
    entry = {"images": n, "rounds": rounds, "same_bytes": bool(same), "loop_spread_max_over_min": round(max(sec["loop"]) / min(sec["loop"]), 3)}
    for k, v in sec.items():
        med = statistics.median(v)
        entry[k] = {"images_per_s": round(n / med, 2), "speedup": round(loop / med, 3), "spread_max_over_min": round(max(v) / min(v), 3)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["rrdb", "compact"], choices=["rrdb", "compact"])
    ap.add_argument("--sets", nargs="+", default=["64", "128", "256", "512", "mixed"])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0), "nets": {}}

    def dump():
        txt = json.dumps(res, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(txt + "\n")
        return txt
    for net in args.nets:
        m, what = model(net)
        entry = res["nets"][net] = {"model": what, "sets": {}}
        for name in args.sets:
            entry["sets"][name] = measure(m, image_set(name, args.images), args.batches, args.rounds)
            print(net, name, json.dumps(entry["sets"][name]), flush=True)
            dump()
        entry["sclk_mhz_after"] = shader_clock_mhz()
        m.model.release_workspace()
        del m
        torch.cuda.empty_cache()
    print(dump())


if __name__ == "__main__":
    main()
