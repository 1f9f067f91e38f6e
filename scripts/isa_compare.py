#!/usr/bin/env python3
"""Compare the gfx950 code generation of two builds of the library, kernel by kernel.  No GPU needed.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S  x.hip -o before/x.s     (at the parent commit)
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S  x.hip -o after/x.s      (at the head)
    scripts/isa_compare.py before after

`--build REV_DIR OUT_DIR file.hip ...` runs those compilations for a checkout's csrc directory.  Per mangled kernel symbol the instruction stream
(comments stripped, basic-block labels renumbered) and the resource metadata (.amdhsa_* block + the assembler's register / scratch / LDS / occupancy
summary) are compared; every differing kernel is listed with both sets of figures and as "reordered" when both builds issue the same multiset of
opcodes (only instruction order / register numbering differs) or "changed" otherwise.  Two things that follow from order and numbering alone are not
counted as a change of opcodes: `s_nop` hazard padding (inserted by the assembler's hazard recogniser according to which instructions end up adjacent) and
`s_addk_i32` for `s_add_i32` (the short encoding is chosen when destination and source land in the same register); the instruction column shows them.  `--table` prints the differing kernels as markdown rows.
Exit status 1 when anything differs.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "--cuda-device-only", "-S"]
SUMMARY = ("NumVgprs", "NumAgprs", "TotalNumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def build(csrc, out, files):
    os.makedirs(out, exist_ok=True)
    inc = os.path.join(csrc, "..", "..", "include")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def one(f):
        subprocess.run([hipcc, *FLAGS, f"-I{inc}", f"-I{csrc}", os.path.join(csrc, f), "-o", os.path.join(out, f.replace(".hip", ".s"))], check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(one, files))


def demangle(names):
    try:
        out = subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """-> {symbol: (instruction lines, metadata lines, {summary field: int})}"""
    bodies, meta, summaries = {}, {}, {}
    last, body, block = None, None, None           # most recent function label; its open instruction list; the open .amdhsa_kernel block
    for raw in open(path):
        line = raw.rstrip("\n")
        m = re.match(r"^(_Z\w+):", line)
        if m:
            last = m.group(1)
            body = bodies[last] = []
            summaries[last] = {}
            continue
        m = re.match(r"^\t\.amdhsa_kernel (\S+)", line)
        if m:
            block = meta[m.group(1)] = []
            continue
        if block is not None:
            if line.startswith("\t.end_amdhsa_kernel"):
                block = None
            else:
                block.append(line.strip())
            continue
        if body is not None:
            if line.startswith("\t.section"):
                body = None                                  # the function's code ends where its .rodata descriptor begins
                continue
            code = line.split(";", 1)[0].rstrip()
            if code.strip():
                body.append(re.sub(r"\.L(BB|tmp)\d+", r".L\1", code))   # block labels carry the function's ordinal in the file
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and last and m.group(1) in SUMMARY:
            summaries[last][m.group(1)] = int(m.group(2))
    return {k: (bodies[k], meta[k], summaries[k]) for k in bodies if k in meta}


def opcodes(body):
    ops = (l.split()[0] for l in body if l.startswith("\t") and not l.lstrip().startswith("."))
    return sorted("s_add_i32" if o == "s_addk_i32" else o for o in ops if o != "s_nop")


def main():
    table = "--table" in sys.argv
    if table:
        sys.argv.remove("--table")
    if len(sys.argv) >= 5 and sys.argv[1] == "--build":
        build(sys.argv[2], sys.argv[3], sys.argv[4:])
        return 0
    before, after = sys.argv[1], sys.argv[2]
    bad = 0
    for f in sorted(os.listdir(after)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(before, f)):
            continue
        a, b = parse(os.path.join(before, f)), parse(os.path.join(after, f))
        names = demangle(sorted(set(a) | set(b)))
        same, diff, rows = 0, [], []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                diff.append((k, "only in " + ("before" if k in a else "after")))
            elif a[k][0] == b[k][0] and a[k][1] == b[k][1] and a[k][2] == b[k][2]:
                same += 1
            else:
                what = [w for w, i in (("instructions", 0), ("metadata", 1), ("summary", 2)) if a[k][i] != b[k][i]]
                kind = "reordered" if opcodes(a[k][0]) == opcodes(b[k][0]) else "changed"
                figs = " ".join(f"{s}={a[k][2].get(s)}->{b[k][2].get(s)}" for s in SUMMARY)
                diff.append((k, f"{kind} ({'+'.join(what)}): instr {len(a[k][0])}->{len(b[k][0])} {figs}"))
                pair = lambda s: str(a[k][2].get(s)) if a[k][2].get(s) == b[k][2].get(s) else f"{a[k][2].get(s)} -> {b[k][2].get(s)}"
                n = (f"{len(a[k][0])}" if len(a[k][0]) == len(b[k][0]) else f"{len(a[k][0])} -> {len(b[k][0])}")
                rows.append(f"| `{names[k]}` | {kind} | {n} | {pair('NumVgprs')} | {pair('NumAgprs')} | {pair('TotalNumSgprs')} | {pair('ScratchSize')} | {pair('Occupancy')} |")
        print(f"{f}: {same} identical, {len(diff)} differing (of {len(set(a) | set(b))} kernels)")
        if table and rows:
            print("| kernel | difference | instructions | VGPRs | AGPRs | SGPRs | scratch | occupancy |\n|---|---|---|---|---|---|---|---|")
            print("\n".join(rows))
        for k, why in ([] if table else diff):
            print(f"    {names[k]}\n        {why}")
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
