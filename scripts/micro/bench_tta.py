"""The self-ensemble's gather and blend alone, on the 1080p lattice (1080 x 1920 BGR, 190 tiles of 200 x 200, scale 4, fp16), against the plain gather
and blend eight times over -- the kernels a user would otherwise launch for eight runs -- and, unless --kernels-only, run_u8(tta=True) against eight
run_u8() of a 4x RRDBNet-23 (synthetic weights, device image in, `out=`).

Device events around --reps launches, the two sides alternated window by window, median of --steps windows after --warmup; the rate is the
algorithm's bytes (image + tiles) over that time.  The straight (k < 4) and the transposed (k >= 4) half of the gather are not separate entry points; their
share is read from a kernel trace.  One JSON line per figure.

    python scripts/micro/bench_tta.py [--steps 20] [--warmup 3] [--reps 5] [--kernels-only]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None):
    import tempfile

    import numpy as np
    import torch

    from innfer_amd import lib as L, run as R, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nb", type=int, default=23)
    ap.add_argument("--e2e-steps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    s, (h, w, C) = 4, (1080, 1920, 3)
    img = synth.image_u8(h, w, C, 2)
    d = torch.from_numpy(img).to(dev)
    ps, ys, xs = L.chop_plan(h, w, 200, 0.5)
    n, P = len(ys) * len(xs), ps * s
    stream = torch.cuda.current_stream(dev).cuda_stream
    tiles = torch.empty((8 * n, C, ps, ps), dtype=torch.float16, device=dev)
    hr = torch.from_numpy(synth.uniform((8 * n, C, 64, 64), 3)).to(dev).half().repeat(1, 1, P // 64 + 1, P // 64 + 1)[:, :, :P, :P].contiguous()
    out = torch.empty((h * s, w * s, C), dtype=torch.uint8, device=dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def plain_gather_x8():
        for k in range(8):
            L.lib.innfer_extract_tiles_u8(d.data_ptr(), C, h, w, 0, 200, 0.5, 0, n, tiles[k * n:].data_ptr(), L.F16, stream)

    def plain_blend_x8():
        for k in range(8):
            L.lib.innfer_recompose_u8(hr[k * n:].data_ptr(), L.F16, n, C, P, h, w, 0.5, s, L.F16, 0, out.data_ptr(), stream)

    pairs = {
        "gather": (lambda: L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), C, h, w, 0, 200, 0.5, 0, 0, 0, 2, tiles.data_ptr(), L.F16, stream), plain_gather_x8,
                   img.size + tiles.numel() * 2, 8 * img.size + tiles.numel() * 2),
        "blend": (lambda: L.lib.innfer_recompose_u8_tta(hr.data_ptr(), L.F16, n, C, P, h, w, 0.5, s, L.F16, 0, 0, 0, -1, 0, out.data_ptr(), stream), plain_blend_x8,
                  hr.numel() * 2 + out.numel(), hr.numel() * 2 + 8 * out.numel()),
    }
    L.check(pairs["gather"][0]())
    L.check(pairs["blend"][0]())
    total = {"tta": 0.0, "plain_x8": 0.0}
    for what, (new, old, new_bytes, old_bytes) in pairs.items():
        new(), old()
        torch.cuda.synchronize(dev)
        tn, to = [], []
        for _ in range(a.warmup + a.steps):
            tn.append(window(new))
            to.append(window(old))
        tn, to = float(np.median(tn[a.warmup:])), float(np.median(to[a.warmup:]))
        total["tta"] += tn
        total["plain_x8"] += to
        print(json.dumps({"kernel": what, "tiles": f"8 x {n} x [{C}, {ps if what == 'gather' else P}, {ps if what == 'gather' else P}] fp16", "tta_ms": round(tn, 4),
                          "tta_TBps": round(new_bytes / tn / 1e9, 2), "plain_x8_ms": round(to, 4), "plain_x8_TBps": round(old_bytes / to / 1e9, 2),
                          "tta_over_plain_x8": round(tn / to, 3), "steps": a.steps, "reps": a.reps}), flush=True)
    print(json.dumps({"pair": "gather + blend", "tta_ms": round(total["tta"], 4), "plain_x8_ms": round(total["plain_x8"], 4),
                      "tta_over_plain_x8": round(total["tta"] / total["plain_x8"], 3)}), flush=True)
    if a.kernels_only:
        return 0
    del tiles, hr
    torch.cuda.empty_cache()

    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=a.nb, scale=s), 0).items()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "4x_rrdb.pth")
        torch.save(sd, path)
        m = R.Model(path, "infer", s, device=dev)
    forms = {"tta": lambda: m.run_u8(d, out=out, tta=True), "plain_x8": lambda: [m.run_u8(d, out=out) for _ in range(8)]}
    times = {k: [] for k in forms}
    for step in range(2 + a.e2e_steps):
        for k, fn in forms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if step >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"end_to_end": f"run_u8 of 1080p, 4x RRDBNet-{a.nb} fp16 chop, device image", "tta_ms": round(med["tta"], 2), "plain_x8_ms": round(med["plain_x8"], 2),
                      "tta_over_plain_x8": round(med["tta"] / med["plain_x8"], 3), "gather_blend_share_of_tta": round(total["tta"] / med["tta"], 4),
                      "steps": a.e2e_steps}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
