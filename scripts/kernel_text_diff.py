#!/usr/bin/env python3
"""kernel_text_diff.py A.so B.so — are two builds' gfx950 kernels the same?

Unbundles every gfx950 code object of both libraries (as tests/test_codeobj.py
does) and compares, per kernel symbol, the bytes of its function, its kernel
descriptor (all but the distance from the descriptor to the code, which any
change of the link order moves) and its metadata entry (kernarg size, LDS,
private segment, SGPR / VGPR counts, workgroup size, ...).  Prints the kernels that differ, or
`identical: <n> kernels`.  Runs on the CPU and only reads.

A kernel that moved to another object keeps its code but not the distance to
the out-of-line device functions it calls.  For a kernel whose bytes differ,
--mask-calls also compares the disassembly with those pc-relative offsets (the
literals added to s_getpc_b64's result) masked, and says `code equal but for
call offsets` where that is all.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_objects(lib, d):
    """Paths of the library's gfx950 code objects, unbundled into d."""
    fat = os.path.join(d, "fatbin")
    # (with no output file llvm-objcopy rewrites its input in place: give it one)
    _run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "copy.so"))
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for n, s in enumerate(starts):
        b = os.path.join(d, "b%d" % n)
        with open(b, "wb") as fh:
            fh.write(blob[s:starts[n + 1] if n + 1 < len(starts) else len(blob)])
        co = b + ".gfx950.o"
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + b,
                            "--targets=" + TARGET, "--output=" + co], capture_output=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            out.append(co)
    return out


def _mask(disasm):
    """A function's disassembly without addresses, encodings and the literals
    of the add / addc pair behind each s_getpc_b64."""
    lines, arm = [], 0
    for ln in disasm.splitlines():
        m = re.match(r"\s+(\S.*?)\s*//", ln)
        if not m:
            continue
        ins = re.sub(r"\s+", " ", m.group(1))
        if ins.startswith("s_getpc_b64"):
            arm = 2
        elif arm and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
            arm -= 1
        lines.append(ins)
    return lines


def kernels(lib, mask=False):
    """{kernel: {"code": bytes, "kd": bytes, "meta": {...}[, "asm": [...]]}}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            raw = open(co, "rb").read()
            secs = {}   # index -> (address, file offset)
            for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)",
                                 _run("llvm-readelf", "-S", "--wide", co), re.M):
                secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
            syms = {}   # name -> bytes
            for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)",
                                 _run("llvm-readelf", "-s", "--wide", co), re.M):
                addr, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(5)
                off = addr - secs[ndx][0] + secs[ndx][1]
                syms[name] = raw[off:off + size]
            for block in _run("llvm-readelf", "--notes", co).split("\n  - .")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if not name or name.group(1) + ".kd" not in syms:
                    continue
                k = name.group(1)
                if k in out:   # (two objects compiled the same kernel, as a header's non-template one)
                    raise SystemExit("%s: kernel %s is in more than one code object" % (lib, k))
                meta = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", block, re.M))
                meta["args"] = re.findall(r"\.(?:offset|size|value_kind|address_space):\s+(\S+)", block)
                # (bytes 16-23 of the descriptor: the distance to the code, which follows the link order)
                kd = syms[k + ".kd"]
                out[k] = {"code": syms[k], "kd": kd[:16] + kd[24:], "meta": meta}
                if mask:
                    out[k]["asm"] = _mask(_run("llvm-objdump", "-d", "--disassemble-symbols=" + k, co))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--mask-calls", action="store_true", help="compare differing code with call offsets masked")
    args = ap.parse_args()
    A, B = kernels(args.a), kernels(args.b)
    bad = 0
    for k in sorted(set(A) ^ set(B)):
        print("only in %s: %s" % (args.a if k in A else args.b, k))
        bad += 1
    differ = [k for k in sorted(set(A) & set(B)) if A[k] != B[k]]
    if differ and args.mask_calls:
        MA, MB = kernels(args.a, True), kernels(args.b, True)
    for k in differ:
        what = [f for f in ("code", "kd", "meta") if A[k][f] != B[k][f]]
        if what == ["code"] and args.mask_calls and len(A[k]["code"]) == len(B[k]["code"]) and \
                MA[k]["asm"] == MB[k]["asm"]:
            print("code equal but for call offsets (%d instructions, descriptor and metadata identical): %s"
                  % (len(MA[k]["asm"]), k))
            continue
        bad += 1
        print("differs in %s: %s" % (", ".join(what), k))
        if "meta" in what:
            for f in sorted(set(A[k]["meta"]) | set(B[k]["meta"])):
                if A[k]["meta"].get(f) != B[k]["meta"].get(f):
                    print("    .%s: %s -> %s" % (f, A[k]["meta"].get(f), B[k]["meta"].get(f)))
    if not bad:
        print("identical: %d kernels%s" % (len(A), "" if not differ else
                                           " (%d of them but for call offsets)" % len(differ)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
