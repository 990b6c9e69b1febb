#!/usr/bin/env python3
"""Device-code diff of two source trees: which gfx950 kernels a change added, removed or changed.

    python tools/kernel_isa_diff.py TREE_A TREE_B        (exit code 1 if any kernel differs)

Every duodiff_amd/csrc/*.hip of both trees is compiled to device assembly with build.py's flags (tools/isa_audit_lds_dma.py's compile_one:
hipcc -S --cuda-device-only, CPU only) and split by function symbol.  Per symbol, the instruction stream (labels and instructions, comments
and directives dropped) and the .amdhsa_kernel descriptor block (registers, LDS, kernarg size, ...) are compared as text.  Only the
numbers of local labels are normalised -- .LBB<n>_, .Ltmp<n>, .Lfunc_end<n> count functions in the order the unit instantiates them,
which a host-side change may permute without touching any kernel.  A refactor of host code, or of a kernel source that claims not to
change the device code, is held to: nothing added, nothing removed, nothing changed.
"""
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from isa_audit_lds_dma import compile_one, instructions, kernels  # noqa: E402

LOCAL = re.compile(r"\.(LBB|Ltmp|Lfunc_end)\d+")


def device_code(tree):
    """{unit: symbol: (instruction text, descriptor text)} of one tree"""
    srcs = sorted((Path(tree) / "duodiff_amd" / "csrc").glob("*.hip"))
    if not srcs:
        sys.exit(f"{tree}: no duodiff_amd/csrc/*.hip")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=4) as ex:
        compiled = list(ex.map(lambda s: compile_one(s, tmp), srcs))
    code = {}
    for src, lines in compiled:
        desc, cur = {}, None
        for l in lines:
            t = l.split(";")[0].strip()
            if t.startswith(".amdhsa_kernel "):
                cur = t.split()[1]
                desc[cur] = []
            elif t == ".end_amdhsa_kernel":
                cur = None
            elif cur and t:
                desc[cur].append(" ".join(t.split()))
        for sym, body in kernels(lines):
            text = "\n".join(LOCAL.sub(r".\1", " ".join(t.split())) for _, t in instructions(body))
            code[f"{src.name}: {sym}"] = (text, "\n".join(desc.get(sym, [])))
    return code


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = device_code(argv[1]), device_code(argv[2])
    added, removed = sorted(set(b) - set(a)), sorted(set(a) - set(b))
    changed = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for title, names in (("added", added), ("removed", removed), ("changed", changed)):
        for k in names:
            what = "" if title != "changed" else " (instructions)" if a[k][0] != b[k][0] else " (descriptor)"
            print(f"{title}: {k}{what}")
    n_desc = sum(1 for v in b.values() if v[1])
    print(f"{len(a)} functions in {argv[1]}, {len(b)} in {argv[2]} ({n_desc} kernels with a descriptor): "
          f"{len(added)} added, {len(removed)} removed, {len(changed)} changed")
    return 1 if added or removed or changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
