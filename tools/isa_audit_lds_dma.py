#!/usr/bin/env python3
"""ISA audit of the M0 wait state in front of every LDS-DMA instruction (duodiff_amd/csrc/*.hip, gfx950).

An LDS-DMA request (`global_load_lds_*`, `buffer_load_* ... lds`) takes its LDS destination from M0.  On GFX9-family parts, gfx950
included, an SALU write of M0 needs one wait state before an LDS-DMA instruction reads it; with none, the request may use the OLD M0 and
land its 1 KB piece in another piece's LDS slot (silent corruption).  LLVM's hazard recognizer pads the sites it emits itself
(`s_mov_b32 m0, ...` / `s_nop 0` / the request), but it does not look inside an inline-asm string, so a hand-written
`s_mov_b32 m0, %0` + request pair must carry its own `s_nop 0`.

This script compiles every translation unit with build.py's flags into a private temp dir and walks each kernel's instruction stream:
an LDS-DMA instruction whose previous instruction writes M0 from the SALU is a finding.  Labels and branches are treated conservatively:
a basic block that starts with the request inherits the last non-branch instruction of EVERY predecessor (fall-through and branch
sources), i.e. a branch is not counted as a wait state.

    python tools/isa_audit_lds_dma.py            (one line per kernel that issues LDS-DMA; exit code 1 on a finding)
"""
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from duodiff_amd.build import FLAGS, hipcc, sources  # noqa: E402

DMA = re.compile(r"^(global_load_lds_\w+|scratch_load_lds_\w+|buffer_load_\w+\b.*\blds\b)")
M0_WRITE = re.compile(r"^s_\w+\s+m0\s*,")                  # SALU instruction whose destination is M0
BRANCH = re.compile(r"^s_(branch|cbranch_\w+)\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def instructions(body):
    """(kind, text) stream of one function: kind 'label' or 'insn'; comments, directives and asm markers dropped"""
    out = []
    for line in body:
        t = line.split(";")[0].strip()
        if not t:
            continue
        m = LABEL.match(t)
        if m:
            out.append(("label", m.group(1)))
        elif not t.startswith(".") and not t.endswith(":"):
            out.append(("insn", t))
    return out


def audit(body):
    """-> (LDS-DMA instructions, findings [(index of the request, the M0 write in front of it)])"""
    ev = instructions(body)
    # basic blocks: a label starts one, a branch or s_endpgm ends one
    blocks, cur = [], {"label": None, "insns": [], "succ": None}
    for kind, t in ev:
        if kind == "label":
            if cur["insns"] or cur["label"]:
                blocks.append(cur)
            cur = {"label": t, "insns": [], "succ": None}
            continue
        cur["insns"].append(t)
        mb = BRANCH.match(t)
        if mb or t.startswith("s_endpgm") or t.startswith("s_setpc_b64"):
            cond = mb is not None and mb.group(1) != "branch"
            cur["succ"] = ([mb.group(2)] if mb else []) + (["<next>"] if cond else [])
            blocks.append(cur)
            cur = {"label": None, "insns": [], "succ": None}
    if cur["insns"] or cur["label"]:
        blocks.append(cur)
    index = {b["label"]: n for n, b in enumerate(blocks) if b["label"]}
    preds = [[] for _ in blocks]
    for n, b in enumerate(blocks):
        for s in (b["succ"] if b["succ"] is not None else ["<next>"]):
            m = n + 1 if s == "<next>" else index.get(s)
            if m is not None and m < len(blocks):
                preds[m].append(n)

    def tails(n, seen):
        """last non-branch instructions reaching the end of block n (through empty blocks)"""
        if n in seen:
            return []
        seen.add(n)
        body_ = [t for t in blocks[n]["insns"] if not BRANCH.match(t)]
        if body_:
            return [body_[-1]]
        return [t for p in preds[n] for t in tails(p, seen)]

    n_dma, findings = 0, []
    for n, b in enumerate(blocks):
        for i, t in enumerate(b["insns"]):
            if not DMA.match(t):
                continue
            n_dma += 1
            prev = [b["insns"][i - 1]] if i > 0 else [x for p in preds[n] for x in tails(p, set())]
            bad = [p for p in prev if M0_WRITE.match(p)]
            if bad:
                findings.append((n_dma, bad[0], t))
    return n_dma, findings


def compile_one(src, tmp):
    out = Path(tmp) / (src.stem + ".s")
    cmd = [hipcc(), *FLAGS, "-S", "--cuda-device-only", str(src), "-o", str(out)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return src, out.read_text().split("\n")


def kernels(lines):
    """(symbol, body lines) of every function in a device assembly file"""
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s*(;.*)?$", l)
        if not m or m.group(1).startswith(".L"):
            continue
        end = next((j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end")), None)
        if end is not None:
            yield m.group(1), lines[i + 1:end]


def main():
    with tempfile.TemporaryDirectory() as tmp:    # private to this run: concurrent runs and other users never collide on it
        with ThreadPoolExecutor(max_workers=4) as ex:
            compiled = list(ex.map(lambda s: compile_one(s, tmp), sources()))
    total_dma = total_bad = 0
    for src, lines in compiled:
        f_dma = f_bad = 0
        for name, body in kernels(lines):
            n_dma, bad = audit(body)
            if not n_dma:
                continue
            f_dma += n_dma
            f_bad += len(bad)
            print(f"{src.name}: {name}: {n_dma} LDS-DMA, {len(bad)} right behind an SALU write of M0:", "OK" if not bad else "FAILED")
            for k, m0, req in bad[:2]:
                print(f"    request #{k}: `{m0}` directly followed by `{req}`")
        print(f"{src.name}: {f_dma} LDS-DMA instructions, {f_bad} findings")
        total_dma += f_dma
        total_bad += f_bad
    print(f"total: {total_dma} LDS-DMA instructions, {total_bad} findings")
    return 1 if total_bad else 0


if __name__ == "__main__":
    sys.exit(main())
