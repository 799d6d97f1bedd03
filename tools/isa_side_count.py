#!/usr/bin/env python3
"""profiles/conv_f32_isa_counts.json: what the compiler emits beside the MFMAs of every conv_f32_kernel instantiation.

conv_f32.hip is compiled device-only to gfx950 assembly with the command the Makefile would run for conv_f32.o
(`make -n`), needing no GPU.  Every instantiation unrolls four stage bodies (two accumulator sets x {first chunk of
a tile, later chunk}) of NSTEP x MT x NT MFMAs each inside the loop over tiles; the first-chunk bodies also carry the
previous tile's epilogue.  Per instantiation:

  steady_side    side instructions of one pass of the loop over a tile's later chunks: a later-chunk body and the
                 chunk loop's own instructions around it (steady_between_mfmas: from the body's first MFMA to its last)
  epilogue_side  side instructions of one tile's pass through the loop over tiles, less one later chunk: the
                 first-chunk body and everything else that runs once per tile, wherever the optimiser put it
  side_per_mfma  (epilogue_side + (NCHUNK - 1) x steady_side) / (NCHUNK x MFMAs per stage): per tile, as it runs
  packed_f32     v_pk_*_f32 anywhere in the kernel
  vgpr_count, vgpr_spill_count, private_segment_size from the code object's metadata

A side instruction is anything a wavefront issues that is neither an MFMA nor scalar ALU / control; s_waitcnt, s_nop
and s_barrier count as side instructions.  The `parent` section is made the same way from another commit's sources
(--parent REV); without --parent the one already in the file is kept.  The stamp (sha16 of conv_f32.hip and of the
Makefile) is what tests/test_conv_f32_isa_counts.py holds the file to.

usage: tools/isa_side_count.py [--parent REV] [--this-asm X.s] [--parent-asm Y.s] > profiles/conv_f32_isa_counts.json"""
import argparse
import hashlib
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join("sp_orb_slam_amd", "csrc")
STAMPED = ("conv_f32.hip", "Makefile")
ARGS = ("LAYER", "CIN", "KS", "KC", "WM", "WN", "MT", "NT", "POOL", "RELU")
COUNTED_SCALAR = ("s_waitcnt", "s_nop", "s_barrier")
CLASSES = (("waitcnt", r"s_waitcnt"), ("nop", r"s_nop"), ("barrier", r"s_barrier"), ("ds_read", r"ds_read"),
           ("ds_write", r"ds_write"), ("load", r"buffer_load|global_load"), ("store", r"buffer_store|global_store"),
           ("accvgpr", r"v_accvgpr"), ("mov", r"v_mov|v_pk_mov"))


def sha16(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def stamp(root):
    return {s: sha16(os.path.join(root, CSRC, s)) for s in STAMPED}


def compile_asm(root, out):
    """the Makefile's own command for conv_f32.o, turned into a device-only assembly listing"""
    csrc = os.path.join(root, CSRC)
    dry = subprocess.run(["make", "-n", "-B", "conv_f32.o"], cwd=csrc, capture_output=True, text=True, check=True).stdout
    line = [l for l in dry.splitlines() if "conv_f32.hip" in l and " -c " in l][-1]
    cmd = shlex.split(line)
    cmd = cmd[:cmd.index("-o")] + cmd[cmd.index("-o") + 2:]
    cmd[cmd.index("-c")] = "-S"
    subprocess.run(cmd + ["--cuda-device-only", "-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)


def template_args(symbol):
    m = re.match(r"_ZN4spfe15conv_f32_kernelI((?:L[ib]\d+E){10})E", symbol)
    return dict(zip(ARGS, [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))])) if m else None


def is_side(op):
    return not op.startswith("v_mfma") and (not op.startswith("s_") or op.split()[0] in COUNTED_SCALAR)


def classify(ops):
    c = {name: 0 for name, _ in CLASSES}
    c["valu_other"] = 0
    for op in ops:
        for name, pat in CLASSES:
            if re.match(pat, op):
                c[name] += 1
                break
        else:
            c["valu_other"] += 1
    return {k: v for k, v in c.items() if v}


def basic_blocks(lines):
    """(label comment, opcodes) per basic block, in layout order"""
    blocks, note, cur = [], "", []
    for l in lines:
        if re.match(r"\.LBB\d+_\d+:|; %bb\.\d+:", l):
            if cur:
                blocks.append((note, cur))
            note, cur = l, []
            continue
        if l.startswith("  ") and ";" in l and not cur:   # the loop notes that continue a label's comment
            note += l
            continue
        m = re.match(r"\t([a-z][a-z0-9_]+)(?:\s+(\.LBB\d+_\d+))?", l)
        if m:
            cur.append(m.group(1) + (" " + m.group(2) if m.group(2) else ""))
    if cur:
        blocks.append((note, cur))
    return blocks


def chunk_pass(blocks, body, others):
    """side opcodes of one pass of the loop over a tile's later chunks: the blocks of the later-chunk body `body` and the
    lightest way through the flow graph from its end back to its start that enters no other stage body"""
    index = {re.match(r"(\.LBB\d+_\d+):", n).group(1): k for k, (n, _) in enumerate(blocks) if n.startswith(".LBB")}
    banned = {k for f in others for k in range(f[0], f[1] + 1)}

    def successors(k):
        ops = blocks[k][1]
        out = [index[op.split()[1]] for op in ops if op.startswith(("s_cbranch", "s_branch")) and " " in op]
        if not (ops and ops[-1].startswith(("s_branch", "s_endpgm"))) and k + 1 < len(blocks):
            out.append(k + 1)
        return out

    cost = lambda k: sum(is_side(op) for op in blocks[k][1])
    best, todo = {}, [(0, s2, ()) for s2 in successors(body[1])]
    while todo:
        todo.sort()
        d, k, path = todo.pop(0)
        if k == body[0]:
            return [op for j in list(range(body[0], body[1] + 1)) + list(path) for op in blocks[j][1] if is_side(op)]
        if k in banned or body[0] < k <= body[1] or best.get(k, 1 << 30) <= d:
            continue
        best[k] = d
        todo += [(d + cost(k), s2, path + (k,)) for s2 in successors(k)]
    raise SystemExit("no way back to the start of a later-chunk body: not a loop over chunks")


def stage_bodies(blocks, per_stage):
    """runs of blocks that hold `per_stage` MFMAs, the unrolled stage bodies -> (first block, last block, side opcodes)"""
    bodies, run, n, first = [], [], 0, 0
    for k, (_, b) in enumerate(blocks):
        nm = sum(op.startswith("v_mfma") for op in b)
        if nm == 0 and n == 0:
            continue
        if n == 0:
            first = k
        run += b
        n += nm
        if n >= per_stage:
            if n == per_stage:   # from the first MFMA to the last: what stands before and behind belongs to the loops around
                at = [k2 for k2, op in enumerate(run) if op.startswith("v_mfma")]
                bodies.append((first, k, [op for op in run[at[0]:at[-1]] if is_side(op)]))
            run, n = [], 0
    return bodies


def loop_of(note, depth):
    """name of the loop of that depth a block's label comment puts it in"""
    if re.search(r"Loop Header: Depth=%d\b" % depth, note):
        return re.match(r"\.L(BB\d+_\d+):", note).group(1)
    m = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+) Depth=%d\b" % depth, note)
    return m.group(1) if m else None


def loop_span(blocks, inside, depth):
    """block range, in layout order, of the loop of that depth around block `inside`"""
    name = loop_of(blocks[inside][0], depth)
    if name is None and depth == 1:   # a block of an inner loop names only that one: ask the inner loop's header
        name = loop_of(blocks[loop_span(blocks, inside, 2)[0]][0], 1)
    members = [k for k in range(len(blocks)) if loop_of(blocks[k][0], depth) == name]
    return min(members), max(members)


def side_of(blocks, lo, hi):
    return [op for _, b in blocks[lo:hi + 1] for op in b if is_side(op)]


def count(asm_path):
    text = open(asm_path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text.split("amdhsa.kernels:")[1])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    out = {}
    for m in re.finditer(r"^(_ZN4spfe15conv_f32_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        sym, body = m.group(1), m.group(2)
        t = template_args(sym)
        if t is None:
            continue
        nchunk, nstep = t["CIN"] // t["KC"], t["KS"] * t["KS"] * (t["KC"] // 2)
        per_stage = nstep * t["MT"] * t["NT"]
        blocks = basic_blocks(body.split("\n"))
        found = stage_bodies(blocks, per_stage)
        if len(found) != 4:
            raise SystemExit("%s: %d stage bodies of %d MFMAs found, 4 expected" % (sym, len(found), per_stage))
        found.sort(key=lambda f: len(f[2]))
        steady = found[1][2]
        # the loop over tiles (one pass = two tiles, one per accumulator set) and, inside it, one pass of the loop over a
        # tile's later chunks
        t_lo, t_hi = loop_span(blocks, min(f[0] for f in found), 1)
        loop = side_of(blocks, t_lo, t_hi)
        chunk_side = len(chunk_pass(blocks, found[1], found[2:] + found[:1]))
        # one tile's pass less one later chunk: the first stage with the epilogue slices in it and whatever else runs once
        # per tile (an epilogue the optimiser hoisted in front of the stages is counted here)
        epi_side = len(loop) // 2 - chunk_side
        key = "<%s>" % ",".join(str(t[a]) for a in ARGS)
        out[key] = {
            "nstep": nstep, "nchunk": nchunk, "mfma_per_stage": per_stage,
            "steady_side": chunk_side, "steady_between_mfmas": len(steady), "steady_classes": classify(steady),
            "epilogue_side": epi_side, "tile_loop_classes": classify(loop),
            "side_per_mfma": round((epi_side + (nchunk - 1) * chunk_side) / (nchunk * per_stage), 4),
            "packed_f32": len(re.findall(r"^\tv_pk_\w+_f32\b", body, re.M)),
            "vgpr_count": meta[sym]["vgpr_count"], "vgpr_spill_count": meta[sym]["vgpr_spill_count"],
            "private_segment_size": meta[sym]["private_segment_fixed_size"],
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="commit whose conv_f32.hip and Makefile make the `parent` section")
    ap.add_argument("--this-asm", help="an assembly listing of this tree's conv_f32.hip, made as compile_asm() does")
    ap.add_argument("--parent-asm")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "conv_f32_isa_counts.json"))
    a = ap.parse_args()
    out = {"what": "side instructions per wavefront beside the MFMAs of conv_f32_kernel (tools/isa_side_count.py)",
           "arguments": list(ARGS)}
    with tempfile.TemporaryDirectory() as tmp:
        if a.parent:
            subprocess.run("git -C %s archive %s %s include | tar -x -C %s" % (shlex.quote(ROOT), shlex.quote(a.parent), CSRC, tmp),
                           shell=True, check=True)
            asm = a.parent_asm or os.path.join(tmp, "parent.s")
            if not a.parent_asm:
                compile_asm(tmp, asm)
            rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], capture_output=True, text=True).stdout.strip()
            out["parent"] = {"commit": rev, "source_sha16": stamp(tmp), "kernels": count(asm)}
        else:
            out["parent"] = json.load(open(a.json))["parent"]
        asm = a.this_asm or os.path.join(tmp, "this.s")
        if not a.this_asm:
            compile_asm(ROOT, asm)
        out["this"] = {"source_sha16": stamp(ROOT), "kernels": count(asm)}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
