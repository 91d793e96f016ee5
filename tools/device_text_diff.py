"""Dev tool (CPU): is the gfx950 device code of two builds the same, object by object?  `python tools/device_text_diff.py <other .build directory> [this .build directory]`
extracts the gfx950 code object of every object on the library's link line (the method of tools/kernel_resources.py) and compares it twice: the bytes of its .text
section (the instructions), and the WHOLE code object — kernel descriptors and metadata included, which hold what the instructions do not show: the register, scratch
and LDS numbers of every kernel.  Prints both verdicts per object and exits non-zero when anything differs.
A change gated to some instantiations must leave every other object "same" (DESIGN.md sections 19 and 25); an edit that only moves or documents source must leave
every object "same" in both columns.    (needs /opt/rocm/lib/llvm/bin/llvm-objcopy)"""
import hashlib, os, struct, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, ROOT, linked_objects


def device_code(obj):
    """(bytes of .text, bytes of the whole gfx950 code object) of the object (None: no such code object)"""
    with tempfile.TemporaryDirectory() as td:
        fat, co, txt = (os.path.join(td, n) for n in ("fat.bin", "dev.co", "text.bin"))
        if subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], capture_output=True).returncode or not os.path.exists(fat):
            return None
        d = open(fat, "rb").read()
        if d[:24] != b"__CLANG_OFFLOAD_BUNDLE__":
            return None
        p = 32
        for _ in range(struct.unpack("<Q", d[24:32])[0]):
            off, size, tl = struct.unpack("<QQQ", d[p:p + 24]); p += 24
            t = d[p:p + tl].decode(); p += tl
            if "gfx950" in t and size:
                whole = d[off:off + size]
                open(co, "wb").write(whole)
                if subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, txt], capture_output=True).returncode or not os.path.exists(txt):
                    return b"", whole  # (a code object without kernels: host-only translation unit)
                return open(txt, "rb").read(), whole
        return None


if __name__ == "__main__":
    other = sys.argv[1]
    mine = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "path_optimizer_amd", "csrc", ".build")
    differ = {".text": [], "code object": []}
    h = lambda v: "-" if v is None else f"{len(v):8d} B {hashlib.sha256(v).hexdigest()[:12]}"
    for base in sorted(linked_objects()):
        a, b = device_code(os.path.join(other, base)), device_code(os.path.join(mine, base))
        if a is None and b is None:
            print(f"{base:28s} no device code")
            continue
        for k, what in enumerate(differ):
            va, vb = (None if a is None else a[k]), (None if b is None else b[k])
            if va != vb:
                differ[what].append(base)
            print(f"{base if k == 0 else '':28s} {what:11s} {'same  ' if va == vb else 'DIFFER'} {h(va)} | {h(vb)}")
    for what, names in differ.items():
        print(f"{what}: {len(names)} differ: {' '.join(names)}")
    sys.exit(1 if any(differ.values()) else 0)
