#!/usr/bin/env python3
"""Per-loop instruction mix of one kernel in a hipcc -S dump.

    tools/isa_loops.py file.s <kernel name substring> [out.json]

A loop is what lies between a backward branch and its target (the blocks from the target label to the branching one, summed in the
manner of tools/isa_blocks.py); nested loops are reported each on its own.  Every instruction is one of VALU / MFMA / accvgpr / LDS /
nop / wait / scratch / other; mfma_adjacent counts the matrix-core products whose next instruction is another product (no
instruction issued in the gap between them).  Counted next to the kinds, per loop and in total: vmem_load (global_load / flat_load /
buffer_load: a vector-memory round trip), vmcnt_wait (an s_waitcnt with a vmcnt field: it waits for such a load, or for the acknowledgement
of a store) and canon_max (v_max_f64 x, y, y: the copy that quiets an operand of a maximum or minimum).  Also printed: the kernel's register counts and private segment, and the totals of the whole kernel.
The self-looping blocks that hold v_mfma_f64 are the tile sweeps of mpc_wave.hpp (tile_factor, tile_forward twice, tile_rhs)."""
import collections
import json
import re
import sys

KINDS = ("valu", "mfma", "accvgpr", "lds", "nop", "wait", "scratch", "other")
EXTRA = ("vmem_load", "vmcnt_wait", "canon_max")      # counted on top of the kinds (each such instruction has a kind as well)


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "accvgpr"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "lds"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("v_"):
        return "valu"
    return "other"


def extras(op, text):
    """the EXTRA counters one instruction line adds to"""
    out = []
    if op.startswith(("global_load", "flat_load", "buffer_load")):
        out.append("vmem_load")
    if op.startswith("s_waitcnt") and "vmcnt" in text:
        out.append("vmcnt_wait")
    if op.startswith("v_max_f64"):
        args = [a.strip() for a in text[len(op):].split(",")]
        if len(args) == 3 and args[1] == args[2]:
            out.append("canon_max")
    return out


def kernel_lines(lines, pat):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and pat in l)
    end = next(i for i in range(start + 1, len(lines)) if ".end_amdhsa_kernel" in lines[i] or re.match(r"^_Z\w*:", lines[i]))
    return lines[start].split(":")[0], lines[start + 1:end]


def parse_blocks(body):
    """[(label, Counter of kinds, [branch targets])] in program order; inline-asm text counts like any other line"""
    blocks = [["entry", collections.Counter(), []]]
    prev = None
    for l in body:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            blocks.append([m.group(1), collections.Counter(), []])
            prev = None
            continue
        if not t or t.startswith((".", "//")) or t.endswith(":"):
            continue
        op = t.split()[0]
        kind = classify(op)
        blocks[-1][1][kind] += 1
        blocks[-1][1]["instrs"] += 1
        for x in extras(op, t):
            blocks[-1][1][x] += 1
        if kind == "mfma" and prev == "mfma":
            blocks[-1][1]["mfma_adjacent"] += 1
        prev = kind
        if op.startswith(("s_cbranch", "s_branch")):
            blocks[-1][2].append(t.split()[-1])
    return blocks


def loops_of(blocks):
    index = {b[0]: i for i, b in enumerate(blocks)}
    out = []
    for i, (label, _, targets) in enumerate(blocks):
        for tgt in targets:
            if tgt in index and index[tgt] <= i:
                tot = collections.Counter()
                for b in blocks[index[tgt]:i + 1]:
                    tot.update(b[1])
                out.append({"head": tgt, "tail": label, "blocks": i + 1 - index[tgt], "self_loop": tgt == label,
                            **{k: tot[k] for k in ("instrs",) + KINDS + ("mfma_adjacent",) + EXTRA}})
    return out


def resources(lines, name):
    res = {}
    for key in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size"):
        m = next((re.search(r",\s*(\d+)\s*$", l) for l in lines if l.strip().startswith(f".set {name}.{key},")), None)
        if m:
            res[key] = int(m.group(1))
    return res


def analyse(path, pat):
    lines = open(path).read().split("\n")
    name, body = kernel_lines(lines, pat)
    blocks = parse_blocks(body)
    tot = collections.Counter()
    for b in blocks:
        tot.update(b[1])
    loops = loops_of(blocks)
    return {"kernel": name, "resources": resources(lines, name), "total": {k: tot[k] for k in ("instrs",) + KINDS + EXTRA},
            "tile_sweeps": [l for l in loops if l["self_loop"] and l["mfma"]], "loops": loops}


if __name__ == "__main__":
    r = analyse(sys.argv[1], sys.argv[2])
    print(r["kernel"], r["resources"])
    print("total", r["total"])
    for l in r["loops"]:
        print(("sweep " if l["self_loop"] and l["mfma"] else "loop  ") + " ".join(f"{k}={v}" for k, v in l.items()))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            json.dump(r, fh, indent=1)
            fh.write("\n")
