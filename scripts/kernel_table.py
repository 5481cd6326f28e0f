#!/usr/bin/env python
"""Per-kernel resources of one libinnfer_amd.so, or of two side by side (no GPU needed):

    python scripts/kernel_table.py LIB [OTHER_LIB] [--match conv3x3]

VGPRs, SGPRs, static LDS, private segment (AMDGPU metadata note of the gfx950 code objects) and code bytes (the kernel symbol's size).  conv3x3_pc
kernels are named <RPW,NT,NLW,OUT,S9,POLY,TMF,CV,NSI>; a tenth argument (NCW, last present at a1ebe9b) is dropped so that both sides match.
profiles/conv_prune/kernels_before_after.txt is this script's output."""
import argparse
import re
import struct
import subprocess

import msgpack


def code_objects(path):
    blob = open(path, "rb").read()
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob):
        base = m.start()
        (n,) = struct.unpack_from("<Q", blob, base + 24)
        p = base + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield blob[base + off:base + off + size]


def kernels(path):
    """{demangled short name: (vgpr, sgpr, lds, private, code bytes)}"""
    out = {}
    for elf in code_objects(path):
        shoff, = struct.unpack_from("<Q", elf, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
        sec = [struct.unpack_from("<IIQQQQII", elf, shoff + i * shentsize) for i in range(shnum)]      # name, type, flags, addr, offset, size, link, info
        sizes = {}
        for (_, typ, _, _, off, size, link, _) in sec:
            if typ != 2:                                              # SHT_SYMTAB
                continue
            stroff = sec[link][4]
            for q in range(off, off + size, 24):
                st_name, st_info, _, _, _, st_size = struct.unpack_from("<IBBHQQ", elf, q)
                if st_info & 15 == 2:                                 # STT_FUNC
                    end = elf.index(b"\0", stroff + st_name)
                    sizes[elf[stroff + st_name:end].decode()] = st_size
        for (_, typ, _, _, off, size, _, _) in sec:
            if typ != 7:                                              # SHT_NOTE
                continue
            q, end = off, off + size
            while q + 12 <= end:
                namesz, descsz, ntype = struct.unpack_from("<III", elf, q)
                d0 = q + 12 + (namesz + 3) // 4 * 4
                if ntype == 32:                                       # NT_AMDGPU_METADATA
                    for k in msgpack.unpackb(elf[d0:d0 + descsz], raw=False, strict_map_key=False).get("amdhsa.kernels", []):
                        out[k[".name"]] = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"], sizes.get(k[".name"], 0))
                q = d0 + (descsz + 3) // 4 * 4
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, dem):
        d = re.sub(r"\(anonymous namespace\)::|innfer::|^void |\(.*\)$", "", d).replace(" ", "")
        d = re.sub(r"\(innfer::OutMode\)", "", d)
        m = re.match(r"conv3x3_pc<((?:[^,]+,){8}[^,]+),[^,]+>$", d)
        if m:
            d = f"conv3x3_pc<{m.group(1)}>"
        short[d] = out[n]
    return short


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--match", default="conv3x3")
    a = ap.parse_args()
    A = {n: v for n, v in kernels(a.lib).items() if a.match in n}
    B = {n: v for n, v in kernels(a.other).items() if a.match in n} if a.other else None
    fmt = lambda v: "%4d %4d %6d %4d %7d" % v if v else "   -    -      -    -       -"
    print("%-66s %s%s" % ("kernel", "vgpr sgpr    lds priv    code", "   | vgpr sgpr    lds priv    code   note" if B is not None else ""))
    for n in sorted(set(A) | set(B or {})):
        line = "%-66s %s" % (n, fmt(A.get(n)))
        if B is not None:
            x, y = A.get(n), B.get(n)
            note = "removed" if y is None else "new" if x is None else "" if x == y else ("code %+d" % (y[4] - x[4]) if x[:4] == y[:4] else "resources differ")
            line += "   | %s   %s" % (fmt(y), note)
        print(line)
    for tag, T in (("before:" if B is not None else "total:", A), ("after: ", B)):
        if T is not None:
            print("%s %d kernels (%d conv3x3_mfma, %d conv3x3_pc), %d code bytes" % (tag, len(T), sum("conv3x3_mfma" in n for n in T), sum("conv3x3_pc" in n for n in T),
                                                                                     sum(v[4] for v in T.values())))


if __name__ == "__main__":
    main()
