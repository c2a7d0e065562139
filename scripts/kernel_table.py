"""developer aid: one row per gfx950 kernel of a library -- registers, LDS, scratch, workgroup limit and code size -- and, with a
second library, the comparison of the two (a refactor must leave every row as it was).

    python3 scripts/kernel_table.py NEW.so [OLD.so] > profiles/kernel_table.md

Kernels are matched by their unqualified names (template arguments kept, parameter types dropped): a kernel whose argument
struct was renamed has another mangled name and is still the same kernel.

The code objects come out of the library with `llvm-objdump --offloading` (one per translation unit), the rows from
`llvm-readelf --notes` (amdhsa.kernels) and the sizes from the kernel symbols (`llvm-readelf --symbols`)."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".max_flat_workgroup_size"]


def unqualified(symbols):
    """{mangled: name without return type, namespaces and parameter list}, by c++filt"""
    plain = subprocess.check_output(["c++filt", "-p"] + symbols, text=True).split("\n")
    out = {}
    for m, d in zip(symbols, plain):
        d = re.sub(r"^void ", "", d)
        head = d.split("<")[0]
        out[m] = head.split("::")[-1] + d[len(head):]
    return out


def kernels(lib):
    """{kernel name: (vgpr, agpr, sgpr, lds, scratch, max workgroup, code bytes)} over every gfx950 code object of the library"""
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(lib), so)
        subprocess.check_call([LLVM + "llvm-objdump", "--offloading", so], cwd=tmp, stdout=subprocess.DEVNULL)
        for obj in sorted(glob.glob(os.path.join(tmp, "*gfx950*"))):
            notes = subprocess.check_output([LLVM + "llvm-readelf", "--notes", obj], text=True)
            syms = subprocess.check_output([LLVM + "llvm-readelf", "--symbols", "--wide", obj], text=True)
            size = {m.group(2): int(m.group(1)) for m in re.finditer(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M)}
            for block in re.split(r"\n  - ", notes.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0])[1:]:
                val = {k: v for k, v in re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", "    " + block, re.M)}
                name = val[".name"]
                assert name not in rows, "kernel %s in two code objects" % name
                rows[name] = tuple(int(val.get(f, "0")) for f in FIELDS) + (size[name],)
    short = unqualified(sorted(rows))
    assert len(set(short.values())) == len(rows), "two kernels share an unqualified name"
    return {short[name]: row for name, row in rows.items()}


def main():
    new = kernels(sys.argv[1])
    old = kernels(sys.argv[2]) if len(sys.argv) > 2 else None
    head = ["kernel", "vgpr", "agpr", "sgpr", "lds", "scratch", "max wg", "code bytes"] + (["same as before"] if old else [])
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    differ = 0
    for name in sorted(set(new) | set(old or {})):
        row = new.get(name)
        cells = [str(v) for v in row] if row else ["absent"] * 7
        if old is not None:
            same = row == old.get(name)
            differ += not same
            cells.append("yes" if same else "NO: before " + (" ".join(str(v) for v in old[name]) if name in old else "absent"))
        print("| `%s` | " % name + " | ".join(cells) + " |")
    if old is not None:
        print("\n%d kernels, %d differ from the library compared with." % (len(new), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
