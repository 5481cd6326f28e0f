"""Seamless modes end to end and kernel by kernel: 4x RRDBNet-23 (synthetic weights, fp16, chop path) on a 1024 x 1024 BGRA texture
(fit_channels, varying alpha) and on a 1080p BGR frame, each in three forms --

    plain      run_u8(img)                                        (what the texture costs today, with its seam)
    seamless   run_u8(img, seamless='tile')                       (border addressing in the gather, crop window in the blend)
    explicit   crop(run_u8(np.pad(img, 16, 'wrap')))              (what users do today: two more full-image passes on the host)

as host images (numpy in, numpy out: PCIe and the host passes are in the time -- the explicit route only exists there) and, for the first two, as
device images (tensor in, `out=`: GPU time only).  The forms are interleaved round by round; medians, one JSON line per (image, form, residence).

Then the gather and the blend alone (`--kernels-only`: nothing else), the seamless entry points on the image against the plain entry points on the
padded image -- the same kernel at pad 16 / crop 16 and at pad 0 / crop 0 -- at the same shapes on the same box: device events around `--reps`
launches, the pairs alternated, median of `--steps` windows; the rate is the algorithm's bytes (image + tiles) over that time.  `extended_ms` is the
time of the plain and fit entry points: the figure to compare across revisions.

    python scripts/bench_seamless.py [--steps 5] [--warmup 2] [--reps 20]"""
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
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    PAD, s = U.SEAMLESS_PAD, 4
    images = {"texture 1024x1024 BGRA": (synth.image_u8(1024, 1024, 4, 1), True), "frame 1920x1080 BGR": (synth.image_u8(1080, 1920, 3, 2), False)}

    if not a.kernels_only:
        sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=a.nb, scale=s), 0).items()}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "4x_rrdb.pth")
            torch.save(sd, path)
            m = R.Model(path, "infer", s, device=dev)
        for name, (img, fit) in images.items():
            h, w, C = img.shape
            d = torch.from_numpy(img).to(dev)
            out = torch.empty((h * s, w * s, C), dtype=torch.uint8, device=dev)
            forms = {
                ("plain", "host"): lambda: m.run_u8(img, fit_channels=fit),
                ("seamless", "host"): lambda: m.run_u8(img, fit_channels=fit, seamless="tile"),
                ("explicit", "host"): lambda: np.ascontiguousarray(
                    m.run_u8(np.pad(img, ((PAD, PAD), (PAD, PAD), (0, 0)), mode="wrap"), fit_channels=fit)[PAD * s:-PAD * s, PAD * s:-PAD * s]),
                ("plain", "device"): lambda: m.run_u8(d, fit_channels=fit, out=out),
                ("seamless", "device"): lambda: m.run_u8(d, fit_channels=fit, out=out, seamless="tile"),
            }
            times = {k: [] for k in forms}
            for step in range(a.warmup + a.steps):
                for k, fn in forms.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    if step >= a.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
            tiles = {pad: len(L.chop_plan(h + 2 * pad, w + 2 * pad, 200, 0.5)[1]) * len(L.chop_plan(h + 2 * pad, w + 2 * pad, 200, 0.5)[2]) for pad in (0, PAD)}
            for (form, where), ts in times.items():
                med = float(np.median(ts))
                print(json.dumps({"image": name, "form": form, "image_on": where, "model": f"4x RRDBNet-{a.nb} fp16 chop", "ms_median": round(med, 2),
                                  "ms_min": round(min(ts), 2), "vs_plain": round(med / float(np.median(times[("plain", where)])), 3),
                                  "tiles": tiles[0] if form == "plain" else tiles[PAD], "steps": a.steps, "sclk_mhz": sclk_mhz()}), flush=True)
        del m
        torch.cuda.empty_cache()

    # ---- the kernels alone: seamless gather / blend on the image vs the plain entry point on the padded image (same lattice, same tile bytes)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for name, (img, fit) in images.items():
        h, w, C = img.shape
        hp, wp = h + 2 * PAD, w + 2 * PAD
        ps, ys, xs = L.chop_plan(hp, wp, 200, 0.5)
        n, P = len(ys) * len(xs), ps * s
        nt, ct = (2 * n, 3) if fit else (n, C)                 # tiles and channels per tile (fit: colour + alpha tiles)
        d = torch.from_numpy(img).to(dev)
        dp = torch.from_numpy(np.pad(img, ((PAD, PAD), (PAD, PAD), (0, 0)), mode="wrap")).to(dev)
        tiles = torch.empty((nt, ct, ps, ps), dtype=torch.float16, device=dev)
        hr = torch.from_numpy(synth.uniform((nt, ct, 64, 64), 3)).to(dev).half().repeat(1, 1, P // 64 + 1, P // 64 + 1)[:, :, :P, :P].contiguous()
        full = torch.empty((hp * s, wp * s, C), dtype=torch.uint8, device=dev)
        crop = torch.empty((h * s, w * s, C), dtype=torch.uint8, device=dev)
        if fit:
            pairs = {
                "gather": (lambda: L.lib.innfer_extract_tiles_u8_fit_seamless(d.data_ptr(), C, h, w, 0, 200, 0.5, 0, n, 1, PAD, 0, tiles.data_ptr(), L.F16, stream),
                           lambda: L.lib.innfer_extract_tiles_u8_fit(dp.data_ptr(), C, hp, wp, 0, 200, 0.5, 0, n, 1, tiles.data_ptr(), L.F16, stream),
                           "innfer_extract_tiles_u8_fit", h * w * C + tiles.numel() * 2, hp * wp * C + tiles.numel() * 2),
                "blend": (lambda: L.lib.innfer_recompose_u8_fit_seamless(hr.data_ptr(), L.F16, n, P, hp, wp, 0.5, s, L.F16, 0, C, 1, -1, PAD, crop.data_ptr(), stream),
                          lambda: L.lib.innfer_recompose_u8_fit(hr.data_ptr(), L.F16, n, P, hp, wp, 0.5, s, L.F16, 0, C, 1, -1, full.data_ptr(), stream),
                          "innfer_recompose_u8_fit", hr.numel() * 2 + crop.numel(), hr.numel() * 2 + full.numel()),
            }
        else:
            pairs = {
                "gather": (lambda: L.lib.innfer_extract_tiles_u8_seamless(d.data_ptr(), C, h, w, 0, 200, 0.5, 0, n, PAD, 0, tiles.data_ptr(), L.F16, stream),
                           lambda: L.lib.innfer_extract_tiles_u8(dp.data_ptr(), C, hp, wp, 0, 200, 0.5, 0, n, tiles.data_ptr(), L.F16, stream),
                           "innfer_extract_tiles_u8", h * w * C + tiles.numel() * 2, hp * wp * C + tiles.numel() * 2),
                "blend": (lambda: L.lib.innfer_recompose_u8_seamless(hr.data_ptr(), L.F16, n, C, P, hp, wp, 0.5, s, L.F16, 0, PAD, crop.data_ptr(), stream),
                          lambda: L.lib.innfer_recompose_u8(hr.data_ptr(), L.F16, n, C, P, hp, wp, 0.5, s, L.F16, 0, full.data_ptr(), stream),
                          "innfer_recompose_u8", hr.numel() * 2 + crop.numel(), hr.numel() * 2 + full.numel()),
            }
        for what, (new, old, old_name, new_bytes, old_bytes) in pairs.items():
            L.check(new())
            L.check(old())
            torch.cuda.synchronize(dev)
            tn, to = [], []
            for _ in range(a.warmup + a.steps):
                x, y = window(new), window(old)
                tn.append(x)
                to.append(y)
            tn, to = float(np.median(tn[a.warmup:])), float(np.median(to[a.warmup:]))
            print(json.dumps({"image": name, "kernel": what, "tiles": f"{nt} x [{ct}, {ps}, {ps}] fp16" if what == "gather" else f"{nt} x [{ct}, {P}, {P}] fp16",
                              "seamless_ms": round(tn, 4), "seamless_TBps": round(new_bytes / tn / 1e9, 2), "extended": old_name + " on the padded image",
                              "extended_ms": round(to, 4), "extended_TBps": round(old_bytes / to / 1e9, 2), "reps": a.reps, "sclk_mhz": sclk_mhz()}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
