"""Register, scratch and LDS figures of every kernel in a compiled object or shared library, from its gfx950
code-object metadata (no GPU needed).  Prints one line per kernel: demangled name, VGPRs, SGPRs, scratch, LDS.

    python scripts/kernel_regs.py fish-speech_amd/build/fm_rowgemv.hip.o [name substring ...]

Two outputs of it (a parent's build and this tree's) diff line by line."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def code_objects(path, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    data = open(fat, "rb").read()
    out = []
    # a file may hold several bundles (a shared library: one per translation unit)
    for n, m in enumerate(re.finditer(rb"__CLANG_OFFLOAD_BUNDLE__", data)):
        b = data[m.start():]
        cnt = int.from_bytes(b[24:32], "little")
        p = 32
        for _ in range(cnt):
            off, size, tl = (int.from_bytes(b[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
            triple = b[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                co = os.path.join(tmp, f"dev{n}.co")
                open(co, "wb").write(b[off:off + size])
                out.append(co)
    return out


def kernels(co):
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    rows = []
    for blk in txt.split("- .agpr_count:")[1:]:
        def f(key):
            m = re.search(r"\." + key + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        rows.append((f("name"), f("vgpr_count"), f("sgpr_count"), f("private_segment_fixed_size"), f("group_segment_fixed_size")))
    return rows


def main():
    path, subs = sys.argv[1], sys.argv[2:]
    with tempfile.TemporaryDirectory() as tmp:
        rows = [r for co in code_objects(path, tmp) for r in kernels(co)]
    names = [r[0] for r in rows]
    for filt in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            names = subprocess.check_output([filt], input="\n".join(names), text=True).split("\n")
            break
        except OSError:
            pass
    for nm, r in sorted(zip(names, rows)):
        if subs and not any(s in nm for s in subs):
            continue
        print(f"{nm}  vgpr {r[1]} sgpr {r[2]} scratch {r[3]} lds {r[4]}")


if __name__ == "__main__":
    main()
