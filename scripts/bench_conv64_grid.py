#!/usr/bin/env python3
"""How much of the epilogue's residual load is exposed: the 192 -> 64 launch at 1080 x 1920, plane-order panels, act 0, res1 from memory (its own 265 MB tensor), on the
diagnostic library: the 8 x 1 form as shipped, the same with INNFER_ABL=512 (no residual loads: wrong results by construction), and the 2 x 4 grid with the prefetch.
Also the RRDB-end launch (res1 from LDS + res2 from memory) on both grids.  Interleaved rounds; us per launch."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["INNFER_LIB"] = os.path.join(ROOT, "innfer_amd", "lib", "libinnfer_amd_ablate.so")
import numpy as np, torch
import innfer_amd.lib as L
dev = torch.device("cuda:0")
H, W, Cc, K = 1080, 1920, 192, 64
g = H * W * 32
slab = (torch.rand((Cc // 32) * g, device=dev) - 0.5).half()
out = torch.empty(2 * g, dtype=torch.float16, device=dev)
res = [(torch.rand(2 * g, device=dev) - 0.5).half() for _ in range(2)]
w = ((np.random.rand(K, Cc, 3, 3) - 0.5) / np.sqrt(9 * Cc)).astype(np.float32)
packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(K, Cc), dtype=np.uint8)
L.check(L.lib.innfer_pack_conv3x3_rows(w.ctypes.data, K, Cc, 1, packed.ctypes.data))
d_packed = torch.from_numpy(packed).to(dev)
d_bias = torch.zeros(64, device=dev)

def args(kind):
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = out.data_ptr(), g, 0, K
    a.N, a.H, a.W, a.act, a.plane_rows = 1, H, W, 0, 1
    if kind == "mem1":
        a.d_res1, a.res1_group_stride, a.res1_scale = res[0].data_ptr(), g, 0.2
    elif kind == "lds1+res2":
        a.d_res1, a.res1_group_stride, a.res1_scale, a.res1_from_input = slab.data_ptr(), g, 0.2, 1
        a.d_res2, a.res2_group_stride, a.res2_scale = res[1].data_ptr(), g, 0.2
    return a

def time(a, grid, abl, reps=30):
    os.environ["INNFER_ABL"] = str(abl)
    for _ in range(3):
        L.check(L.lib.innfer_conv3x3_f16_grid(C.byref(a), grid, None))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        L.lib.innfer_conv3x3_f16_grid(C.byref(a), grid, None)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps

variants = [("none  8x1", "none", 0, 0), ("none  2x4", "none", 1, 0),
            ("mem1  8x1 shipped", "mem1", 0, 0), ("mem1  8x1 abl512 (no residual loads)", "mem1", 0, 512), ("mem1  2x4 + prefetch", "mem1", 1, 0),
            ("lds1+res2  8x1", "lds1+res2", 0, 0), ("lds1+res2  8x1 abl512", "lds1+res2", 0, 512), ("lds1+res2  2x4 + prefetch", "lds1+res2", 1, 0)]
A = {k: args(k) for k in ("none", "mem1", "lds1+res2")}
rows = {v[0]: [] for v in variants}
for rnd in range(4):
    for name, kind, grid, abl in variants:
        rows[name].append(time(A[kind], grid, abl))
for name, _, _, _ in variants:
    v = rows[name]
    print(f"{name:40s} " + " ".join(f"{x:7.1f}" for x in v) + f"   median {float(np.median(v)):7.1f} us", flush=True)
