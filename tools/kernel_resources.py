#!/usr/bin/env python3
"""Registers / LDS / scratch of every kernel in libdsdiff.so, read from the gfx950 code objects embedded in the library
(no GPU needed): the AMDGPU metadata note of each object via llvm-readelf.
    python tools/kernel_resources.py [--spills]        # --spills: only kernels with scratch or spilled registers
    python tools/kernel_resources.py --digest FILE [--lib PATH]    # name, resource fields, SHA-256 of the machine code
    python tools/kernel_resources.py --compare A B [--report FILE] # two digests: exit 1 unless every kernel is identical
Used by tests/test_abi.py: a kernel that hipcc made spill is a build regression (and, for kernels that keep asm-loaded
registers live, a correctness hazard — DESIGN.md §9).
--digest / --compare prove that a source-only refactor left the machine code alone: the hash covers the kernel's own bytes,
the slice of .text that its FUNC symbol names (value, size), read straight from the ELF."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FIELDS = ("vgpr", "sgpr", "lds", "scratch", "vgpr_spills", "sgpr_spills")


def code_objects(path):
    data = open(path, "rb").read()
    for m in re.finditer(b"\x7fELF\x02\x01\x01", data):
        i = m.start()
        if data[i + 18:i + 20] != b"\xe0\x00":      # e_machine = EM_AMDGPU
            continue
        e_shoff, = struct.unpack_from("<Q", data, i + 0x28)
        e_shentsize, e_shnum = struct.unpack_from("<HH", data, i + 0x3A)
        yield data[i:i + e_shoff + e_shentsize * e_shnum]


def function_bytes(co):
    """{symbol name: its bytes} for every FUNC symbol of one code object (ELF64 little-endian section / symbol tables)."""
    e_shoff, = struct.unpack_from("<Q", co, 0x28)
    e_shentsize, e_shnum = struct.unpack_from("<HH", co, 0x3A)
    # (sh_type, sh_addr, sh_offset, sh_size, sh_link)
    secs = [struct.unpack_from("<4xI8xQQQI", co, e_shoff + k * e_shentsize) for k in range(e_shnum)]
    out = {}
    for typ, _, off, size, link in secs:
        if typ != 2:                                 # SHT_SYMTAB
            continue
        str_off = secs[link][2]
        for s in range(off, off + size, 24):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, s)
            if (st_info & 0xF) != 2 or not 0 < st_shndx < e_shnum:   # STT_FUNC, defined here
                continue
            name = co[str_off + st_name:co.index(b"\0", str_off + st_name)].decode()
            _, addr, soff, _, _ = secs[st_shndx]
            out[name] = co[soff + st_value - addr:soff + st_value - addr + st_size]
    return out


def kernels(path=None, code=False):
    """[{name, vgpr, sgpr, lds, scratch, vgpr_spills, sgpr_spills}] over all code objects of the library; code=True adds
    size and sha256 of each kernel's machine code."""
    path = path or os.path.join(ROOT, "diffusion_models_dsdiff_amd", "libdsdiff.so")
    out = []
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        funcs = function_bytes(co) if code else {}
        for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            def field(k, d=0):
                mm = re.search(r"\." + k + r":\s+(\S+)", blk)
                return mm.group(1) if mm else d
            out.append({"name": field("name", "?"), "vgpr": int(field("vgpr_count")), "sgpr": int(field("sgpr_count")),
                        "lds": int(field("group_segment_fixed_size")), "scratch": int(field("private_segment_fixed_size")),
                        "vgpr_spills": int(field("vgpr_spill_count")), "sgpr_spills": int(field("sgpr_spill_count"))})
            if code:
                body = funcs[out[-1]["name"]]
                out[-1].update(size=len(body), sha256=hashlib.sha256(body).hexdigest())
    return out


def compare(a, b):
    """Differences between two digests, as lines; none = every kernel of a is in b with the same resources and code."""
    def index(ks):
        d = {}
        for k in ks:
            d.setdefault(k["name"], []).append(k)     # (file-local kernels of two translation units may share a name)
        return d
    da, db = index(a), index(b)
    lines = [f"missing: {n}" for n in da if n not in db] + [f"added: {n}" for n in db if n not in da]
    for n in da:
        if n not in db:
            continue
        if len(da[n]) != len(db[n]):
            lines.append(f"count {len(da[n])} -> {len(db[n])}: {n}")
            continue
        key = lambda k: (k["sha256"], k["size"])
        for x, y in zip(sorted(da[n], key=key), sorted(db[n], key=key)):
            diff = [f"{f} {x[f]} -> {y[f]}" for f in FIELDS + ("size", "sha256") if x[f] != y[f]]
            if diff:
                lines.append(f"differs ({', '.join(diff)}): {n}")
    return lines


def main(argv):
    def arg(flag, n=1):
        i = argv.index(flag)
        return argv[i + 1] if n == 1 else argv[i + 1:i + 1 + n]
    if "--compare" in argv:
        pa, pb = arg("--compare", 2)
        a, b = json.load(open(pa))["kernels"], json.load(open(pb))["kernels"]
        lines = compare(a, b)
        if "--report" in argv:
            whole = hashlib.sha256("".join(sorted(k["name"] + k["sha256"] for k in b)).encode()).hexdigest()
            with open(arg("--report"), "w") as f:
                json.dump({"kernels_before": len(a), "kernels_after": len(b), "identical": not lines, "differences": lines,
                           "code_bytes": sum(k["size"] for k in b), "sha256_of_all": whole, "kernels": b}, f, indent=0)
        print("\n".join(lines) if lines else f"{len(b)} kernels: names, resource fields and machine code identical")
        return 1 if lines else 0
    if "--digest" in argv:
        ks = sorted(kernels(arg("--lib") if "--lib" in argv else None, code=True), key=lambda k: (k["name"], k["sha256"]))
        with open(arg("--digest"), "w") as f:
            json.dump({"kernels": ks}, f, indent=0)
        print(f"{len(ks)} kernels, {sum(k['size'] for k in ks)} bytes of code")
        return 0
    ks = kernels()
    only = "--spills" in argv
    print(f"{len(ks)} kernels")
    for k in sorted(ks, key=lambda k: -k["vgpr"]):
        if only and not (k["scratch"] or k["vgpr_spills"] or k["sgpr_spills"]):
            continue
        print(f"{k['vgpr']:4d} vgpr {k['sgpr']:4d} sgpr {k['lds']:7d} lds {k['scratch']:6d} scratch {k['vgpr_spills']:4d}/{k['sgpr_spills']:<4d} spills  {k['name'][:110]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
