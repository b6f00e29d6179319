"""dev: compare two builds of libsanta_hip.so kernel by kernel (no GPU needed).
    python tools/kernel_diff.py OLD.so NEW.so ['NEWTEXT=OLDTEXT' ...]
(a kernel of NEW whose name with NEWTEXT replaced by OLDTEXT exists in OLD is
compared with that one: a template parameter added since OLD)
Unbundles the gfx950 code object of each library, disassembles it and compares
every kernel's instruction stream (addresses and branch-target labels removed)
by demangled name; prints the kernels that differ, that exist on one side
only, and every kernel of NEW with private (scratch) memory."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(lib, tmp, tag):
    fb, co = os.path.join(tmp, tag + ".fb"), os.path.join(tmp, tag + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(tmp, "junk")],
                   check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fb}", f"--output={co}", "--unbundle"], check=True)
    return co


def kernels(co):
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co],
                         check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            x = line.split("//")[0].strip()
            if x == "...":  # the listing's mark for zero padding after the code object's last kernel
                continue
            x = re.sub(r"<[^>]*>", "<L>", x)           # branch-target labels
            x = re.sub(r"(s_c?branch\S*|s_call\S*)\s+\S+", r"\1", x)  # and their offsets
            out[name].append(x)
    return out


def scratch(co):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    res = {}
    for block in re.split(r"\n\s+- \.", notes):
        name = re.search(r"\.?name:\s+(_Z\S+)", block)
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        if name and priv:
            res[name.group(1)] = int(priv.group(1))
    return res


def main():
    old, new = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        co_o, co_n = code_object(old, tmp, "old"), code_object(new, tmp, "new")
        ko, kn = kernels(co_o), kernels(co_n)
        for a in sys.argv[3:]:  # NEW=OLD: compare NEW's kernel named NEW with OLD's named OLD
            n_, o_ = a.split("=")
            kn = {(k.replace(n_, o_) if k.replace(n_, o_) in ko else k): v for k, v in kn.items()}
        same = [k for k in ko if k in kn and ko[k] == kn[k]]
        print(f"{len(same)} kernels identical")
        for k in sorted(ko):
            if k not in kn:
                print("only in OLD:", k)
            elif ko[k] != kn[k]:
                d = [x for x in difflib.unified_diff(ko[k], kn[k], lineterm="", n=0) if x[:1] in "+-"][2:]
                print(f"DIFFERS ({len(ko[k])} -> {len(kn[k])} instructions, {len(d)} diff lines):", k)
                for x in d[:12]:
                    print("   ", x)
        for k in sorted(kn):
            if k not in ko:
                print("only in NEW:", k, f"({len(kn[k])} instructions)")
        sc = scratch(co_n)
        print("kernels of NEW with scratch:", {k: v for k, v in sc.items() if v})
        print("lsap kernels of NEW:", len([k for k in sc if "lsap_" in k]), "all without scratch:",
              not any(v for k, v in sc.items() if "lsap_" in k))


if __name__ == "__main__":
    main()
