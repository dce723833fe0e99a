"""Are the gfx950 kernels of two builds of the library the same code?
    python tools/kcode_diff.py A.so B.so [name-substring]
Takes the gfx950 code objects out of each library (llvm-objcopy, the offload bundles of .hip_fatbin)
and compares, for every kernel symbol, the kernel's machine-code bytes, its kernel descriptor and its
resource metadata (VGPRs, SGPRs, spills, LDS, scratch; llvm-readelf --notes).  One line per kernel:
same / differs (with what) / only in A / only in B; exit status 0 only if every kernel is the same.
Bytes and metadata only: no instruction is decoded.  Needs no GPU.  (A refactor that moves kernels
between files proves with it that it changed none: DESIGN.md section 1.)"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size",
        "uses_dynamic_stack")


def code_objects(lib, tmp):
    """The gfx950 ELF images of a library's fat binary (one per translation unit)."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib,
                    os.path.join(tmp, "copy")], check=True)
    d = open(fat, "rb").read()
    out = []
    at = d.find(MAGIC)
    while at >= 0:  # uncompressed bundle: magic, u64 count, count x {u64 offset, u64 size, u64 len, id}
        (n,) = struct.unpack_from("<Q", d, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", d, p)
            ident = d[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                out.append(d[at + off:at + off + size])
        at = d.find(MAGIC, at + len(MAGIC))
    if not out:
        sys.exit(f"{lib}: no gfx950 code object found (a compressed fat binary is not supported)")
    return out


def kernels_of(elf, tmp):
    """name -> (code bytes, descriptor bytes, metadata dict) of one code object."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2, "not a 64-bit ELF image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]

    def at(addr, size, shndx):  # the bytes of a symbol
        _, typ, _, saddr, soff, _, _, _, _, _ = secs[shndx]
        return b"\0" * size if typ == 8 else elf[soff + addr - saddr:soff + addr - saddr + size]

    syms = {}
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 2:  # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for i in range(size // entsize):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, off + i * entsize)
            if 0 < shndx < shnum:
                end = elf.index(b"\0", stroff + name)
                syms[elf[stroff + name:end].decode()] = (value, ssize, shndx)
    path = os.path.join(tmp, "co.elf")
    open(path, "wb").write(elf)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], check=True, capture_output=True,
                           text=True).stdout
    meta = {}
    for blk in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^    \.(\w+):\s+(\S+)\s*$", "    " + blk, flags=re.M))
        if "symbol" in kv:
            meta[kv["name"]] = {k: kv.get(k) for k in META}
    out = {}
    for name, m in meta.items():
        # Descriptor bytes 16..23 are the distance from the descriptor to the code (where the linker
        # put the two in this code object), not a property of the kernel: left out.
        kd = at(*syms[name + ".kd"])
        out[name] = (at(*syms[name]), kd[:16] + kd[24:], m)
    return out


def kernels(lib):
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        for elf in code_objects(lib, tmp):
            for name, k in kernels_of(elf, tmp).items():
                if name in out:
                    sys.exit(f"{lib}: kernel {name} is defined in two code objects")
                out[name] = k
        return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    names = sorted(n for n in set(a) | set(b) if pat in n)
    for n in names:
        if n not in a or n not in b:
            verdict = "only in A" if n in a else "only in B"
        else:
            (ca, da, ma), (cb, db, mb) = a[n], b[n]
            what = []
            if ca != cb:
                what.append(f"code ({len(ca)} / {len(cb)} bytes)")
            if da != db:
                what.append("descriptor")
            what += [f"{k} {ma[k]} / {mb[k]}" for k in META if ma[k] != mb[k]]
            verdict = "differs: " + ", ".join(what) if what else "same"
        bad += verdict != "same"
        m = (a.get(n) or b[n])[2]
        print(f"{verdict:9s} {n}  [{len((a.get(n) or b[n])[0])} B, vgpr {m['vgpr_count']} sgpr {m['sgpr_count']} "
              f"spill {m['vgpr_spill_count']}+{m['sgpr_spill_count']} lds {m['group_segment_fixed_size']} "
              f"scratch {m['private_segment_fixed_size']}]")
    print(f"{len(names)} kernels, {len(names) - bad} same, {bad} not")
    sys.exit(1 if bad or not names else 0)


if __name__ == "__main__":
    main()
