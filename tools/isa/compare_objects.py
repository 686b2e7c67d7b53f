#!/usr/bin/env python3
"""compare_objects.py -- are the gfx950 kernels of two builds of one object
the same?  Not part of the product.

  python tools/isa/compare_objects.py before/team.o after/team.o

Both objects' gfx950 code objects are taken out the way
tests/test_isa_budget.py does (llvm-objcopy --dump-section=.hip_fatbin,
clang-offload-bundler --unbundle) and disassembled (llvm-objdump -d).  Per
symbol, with the addresses stripped, the instruction streams (mnemonics,
operands and encodings) must be equal; so must the metadata rows of
reg_table.py (VGPRs, AGPRs, SGPRs, scratch, spills, waves per SIMD) and the
LDS bytes.  Prints one line per symbol that differs or exists on one side
only, then the counts; exit status 0 only when nothing differs.
"""
import bisect
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reg_table  # noqa: E402

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(tool, *args, **kw):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, **kw)


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    run("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, tag + ".rest"),
        capture_output=True)
    run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}", capture_output=True)
    return co


def streams(co):
    """symbol -> its instructions without their addresses.  The literal of an
    s_getpc_b64 / s_add_u32 / s_addc_u32 triple (a call of a function that
    was not inlined, a far branch) is an offset from the triple's own address
    and moves with the layout of the code object: it is replaced by the symbol
    and offset it points at."""
    text = run("llvm-objdump", "-d", co, capture_output=True, text=True).stdout
    syms, out, cur = [], {}, None
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            syms.append((int(m.group(1), 16), m.group(2)))
            cur = out.setdefault(m.group(2), [])
        elif cur is not None and line.strip():
            cur.append(line.strip())
    syms.sort()

    def where(addr):
        at = [a for a, _ in syms]
        i = bisect.bisect_right(at, addr) - 1
        return f"<{syms[i][1]}+{addr - syms[i][0]:#x}>" if i >= 0 else f"<{addr:#x}>"

    ins = re.compile(r"^(\S+) (.*?)\s*//\s*([0-9A-Fa-f]+): (.*)$")
    for body in out.values():
        for i, line in enumerate(body):
            m = ins.match(line)
            if not m:
                continue
            body[i] = f"{m.group(1)} {m.group(2)} // {m.group(4)}"
            if m.group(1) == "s_getpc_b64" and i + 2 < len(body):
                lo, hi = ins.match(body[i + 1]), ins.match(body[i + 2])
                if lo and hi and lo.group(1) == "s_add_u32" and hi.group(1) == "s_addc_u32":
                    off = int(lo.group(2).split(",")[-1], 0) + (int(hi.group(2).split(",")[-1], 0) << 32)
                    off -= (off >> 63) << 64
                    dst = where(int(lo.group(3), 16) + off)
                    body[i + 1] = f"s_add_u32 {lo.group(2).rsplit(',', 1)[0]}, lo{dst}"
                    body[i + 2] = f"s_addc_u32 {hi.group(2).rsplit(',', 1)[0]}, hi{dst}"
    return out


def metadata(co, tmp, tag):
    """mangled kernel name -> (reg_table row without the name, LDS bytes)"""
    notes = os.path.join(tmp, tag + ".notes")
    with open(notes, "w") as f:
        run("llvm-readelf", "--notes", co, stdout=f)
    text = open(notes).read()
    lds, names = {}, []
    for item in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", item))
        if "name" in f and not f["name"].endswith(".kd"):
            names.append(f["name"])
            lds[f["name"]] = int(f.get("group_segment_fixed_size", 0))
    rows = reg_table.parse(notes)
    assert len(rows) == len(names)
    return {n: ({k: v for k, v in r.items() if k != "kernel"}, lds[n]) for n, r in zip(names, rows)}


def main():
    before, after = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        ca, cb = code_object(before, tmp, "a"), code_object(after, tmp, "b")
        sa, sb = streams(ca), streams(cb)
        ma, mb = metadata(ca, tmp, "a"), metadata(cb, tmp, "b")
    differ = 0
    for name in sorted(set(sa) | set(sb)):
        if name not in sa or name not in sb:
            verdict = "only in " + (before if name in sa else after)
        elif sa[name] != sb[name]:
            verdict = f"instructions differ ({len(sa[name])} -> {len(sb[name])})"
        elif ma.get(name) != mb.get(name):
            verdict = f"metadata differs ({ma.get(name)} -> {mb.get(name)})"
        else:
            continue
        differ += 1
        print(f"{verdict}: {reg_table.demangle([name])[0]}")
    both = len(set(sa) & set(sb))
    print(f"{before} -> {after}: {len(sa)} / {len(sb)} symbols, {len(ma)} / {len(mb)} kernels with "
          f"metadata, {both} compared, {both + len(set(sa) ^ set(sb)) - differ} identical, "
          f"{differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
