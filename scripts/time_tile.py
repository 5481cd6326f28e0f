"""The stitched tile path against the 200 / 0.5 chop on the MI355X (measurement only; needs the GPU).

(a) Model.run_u8 of 1080 x 1920 and 2160 x 3840 uint8 images with the RRDBNet-23 4x synth model: tile=None (the reference's chop, the code as it was),
    tile=512, tile=1024 and tile=0 (the whole image) alternate in ONE process round by round, host clock around a synchronised call; medians, the ratios
    to tile=None, and next to them what the pixel counts predict (tiles x tile area / image area of each lattice).
(b) the two new uint8 kernels alone at the 4K sizes (tile 512 + 16, scale 4) against innfer_extract_tiles_u8 / innfer_recompose_u8 on the same image:
    device-event time per launch, the four alternate, medians.
The shader clock is read (rocm-smi, read only) after each part.

    python scripts/time_tile.py [--rounds 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from innfer_amd.run import Model    # noqa: E402

SIZES = ((1080, 1920), (2160, 3840))
TILES = (None, 512, 1024, 0)
PAD = 16


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


def pixel_share(H, W, tile):
    """Pixels through the network / pixels of the image."""
    if tile == 0:
        return 1.0
    if tile is None:
        ps, ys, xs = L.chop_plan(H, W, min(H, W, 200), 0.5)
        return ps * ps * len(ys) * len(xs) / (H * W)
    ph, pw, ys, xs = L.tile_plan(H, W, tile, PAD)
    return ph * pw * len(ys) * len(xs) / (H * W)


def name(tile):
    return "chop_200_0.5" if tile is None else f"tile_{tile}"


def images(dev, rounds):
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=23, scale=4), 0).items()}
    m = Model(None, "infer", 4, state_dict=sd, tile_pad=PAD)
    res = []
    for H, W in SIZES:
        img = torch.from_numpy(synth.image_u8(H, W, 3, H)).to(dev)
        out = torch.empty((4 * H, 4 * W, 3), dtype=torch.uint8, device=dev)
        ms, failed = {t: [] for t in TILES}, {}
        for r in range(rounds + 2):                                        # two rounds of warm-up (workspaces, the allocator's blocks)
            for t in TILES:
                if t in failed:
                    continue
                m.tile = t
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    m.run_u8(img, out=out)
                except torch.OutOfMemoryError as e:
                    failed[t] = str(e)[:200]
                    m.model.release_workspace()
                    torch.cuda.empty_cache()
                    continue
                torch.cuda.synchronize()
                if r >= 2:
                    ms[t].append((time.perf_counter() - t0) * 1e3)
        base = statistics.median(ms[None])
        entry = dict(image=f"{H}x{W}", rounds=rounds, paths={})
        for t in TILES:
            e = dict(pixel_share=round(pixel_share(H, W, t), 4), predicted_speedup=round(pixel_share(H, W, None) / pixel_share(H, W, t), 3))
            if t in failed:
                e["failed"] = failed[t]
            else:
                med = statistics.median(ms[t])
                e.update(median_ms=round(med, 2), min_ms=round(min(ms[t]), 2), measured_speedup=round(base / med, 3))
            entry["paths"][name(t)] = e
        res.append(entry)
        m.model.release_workspace()
        del img, out
        torch.cuda.empty_cache()
    return res


def kernels(dev, rounds):
    H, W, s, tile = 2160, 3840, 4, 512
    stream = torch.cuda.current_stream(dev).cuda_stream
    img = torch.from_numpy(synth.image_u8(H, W, 3, 5)).to(dev)
    out = torch.empty((s * H, s * W, 3), dtype=torch.uint8, device=dev)
    ps, cys, cxs = L.chop_plan(H, W, 200, 0.5)
    nc = len(cys) * len(cxs)
    ph, pw, ys, xs = L.tile_plan(H, W, tile, PAD)
    nt = len(ys) * len(xs)
    lr_c = torch.empty((nc, 3, ps, ps), dtype=torch.float16, device=dev)
    lr_t = torch.empty((nt, 3, ph, pw), dtype=torch.float16, device=dev)
    hr_c = torch.rand((nc, 3, s * ps, s * ps), device=dev).half()           # (random data: zeros would read fast)
    hr_t = torch.rand((nt, 3, s * ph, s * pw), device=dev).half()
    runs = {
        "extract_tiles_u8 (200 / 0.5)": lambda: L.check(L.lib.innfer_extract_tiles_u8(img.data_ptr(), 3, H, W, 0, ps, 0.5, 0, nc, lr_c.data_ptr(), L.F16, stream)),
        "extract_tiles_u8_rect (512 + 16)": lambda: L.check(L.lib.innfer_extract_tiles_u8_rect(img.data_ptr(), 3, H, W, 0, tile, PAD, 0, nt, 0, 2, lr_t.data_ptr(), L.F16, stream)),
        "recompose_u8 (200 / 0.5)": lambda: L.check(L.lib.innfer_recompose_u8(hr_c.data_ptr(), L.F16, nc, 3, s * ps, H, W, 0.5, s, L.F16, 0, out.data_ptr(), stream)),
        "stitch_tiles_u8 (512 + 16)": lambda: L.check(L.lib.innfer_stitch_tiles_u8(hr_t.data_ptr(), L.F16, nt, 3, H, W, tile, PAD, s, 0, 0, out.data_ptr(), stream)),
    }
    ms = {k: [] for k in runs}
    for r in range(rounds + 3):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 3:
                ms[k].append(a.elapsed_time(b))
    res = dict(image=f"{H}x{W}", scale=s, tiles=dict(chop=[nc, ps, ps], stitched=[nt, ph, pw]),
               bytes=dict(chop_gather=img.numel() + lr_c.numel() * 2, stitched_gather=img.numel() + lr_t.numel() * 2,
                          chop_blend=hr_c.numel() * 2 + out.numel(), stitched_stitch=hr_t.numel() * 2 + out.numel()))
    res["median_ms"] = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    res["min_ms"] = {k: round(min(v), 4) for k, v in ms.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": "RRDBNet nb 23, 4x, synth weights, fp16 engine", "tile_pad": PAD}
    res["run_u8"] = images(dev, args.rounds)
    res["sclk_mhz_after_run_u8"] = shader_clock_mhz()
    res["kernels_4k"] = kernels(dev, max(20, args.rounds))
    res["sclk_mhz_after_kernels"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
