#!/usr/bin/env python3
"""Code-generation report of the wave-scheduled RTIOW kernels (CPU only: compiles to assembly, runs nothing).
usage: tools/wave_codegen.py [--base OTHER_TREE] [--json] [--only NAME[,NAME..]] [TREE]

For every wave instantiation (headline, work-stealing, indep, moments, and the LDS_SCENE = 3 counting one) a one-kernel translation
unit is compiled with the Makefile's flags plus --cuda-device-only -S.  The kernel's assembly is cut into basic blocks, and for each
scheduler block X of TRAV, LEAF, SHADE, GEN, FILL the PICK PATH  header -> X -> latch -> header  is measured:
    insts   every instruction on the path          valu    the v_* ones among them
    mov     v_mov_b32 / v_mov_b64 / v_accvgpr_*    lane    v_readlane / v_writelane (spilled SGPRs)
The path is the shortest one (in instructions) through the way points that the body marks with RL_CG_MARK comment lines (rl_rtiow_wave.h),
with divergent regions entered: an s_cbranch_execz is not followed, unless it is a lane loop's only exit.  TRAV's path runs its step loop once (two steps);
`step` is the VALU count of one step body on its own, so  valu - 2 * step  is what a TRAV pick costs around its steps.
The kernel's register figures are those tools/kernel_regs.py reads from a built library.
`passes`: the VALU count of ONE block pass of Ring::coop_blocks in each form, FULL (a lane per block, 64 jobs) and QUAD (four lanes per
block, 16 jobs), between their marks, for every copy in the kernel (GEN's, then FILL's), with the rolled round loop (a block that
branches to itself) counted four times; and `quad_max`, the largest remainder R for which ceil(R / 16) quad passes cost fewer VALU
instructions than one full pass, from the first copy: what Ring::COOP_QUAD_MAX must not exceed.

With --base the same report is made for a second tree and printed beside the first (base -> tree).  A tree from before the marks
existed gets them inserted into a temporary copy of its body, at the same places (they are comment lines in the assembly, but a
`volatile` statement all the same: the marked parent's code differs from its library's by a few instructions in five thousand)."""
import argparse
import concurrent.futures
import heapq
import json
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("rendering-learning_amd", "csrc")
INSTANCES = {  # name -> explicit instantiation
    "headline": "rl::rtiow_wave_kernel<1024, 4, false, false>",
    "steal": "rl::rtiow_wave_kernel<1024, 4, false, true>",
    "indep": "rl::rtiow_wave_indep_kernel<1024, 4, false>",
    "moments": "rl::rtiow_wave_moments_kernel<1024, 4>",
    "counting": "rl::rtiow_wave_kernel<1024, 3, true, false>",
}
BLOCKS = ("TRAV", "LEAF", "SHADE", "GEN", "FILL")
MARK_MACRO = '-DRL_CG_MARK(name)=asm volatile("; rl_cg " name)'

# the marks of a body that predates them: (anchor text, replacement) — each anchor occurs exactly once
_OLD_BODY_MARKS = [
    ("  for (;;) {\n    // a finished traversal goes to SHADE;", '  for (;;) {\n    RL_CG_MARK("HEAD");\n    // a finished traversal goes to SHADE;'),
    ("    if (pick == ST_TRAV) {\n      // several steps", '    if (pick == ST_TRAV) {\n      RL_CG_MARK("TRAV_B");\n      // several steps'),
    ("        if (state == ST_TRAV) {\n          // one LDS round trip", '        RL_CG_MARK("STEP_B");\n        if (state == ST_TRAV) {\n          // one LDS round trip'),
    ("            state = w >> 29;\n          }\n        }\n      };\n", '            state = w >> 29;\n          }\n        }\n        RL_CG_MARK("STEP_E");\n      };\n'),
    ("< floor_n) break;\n      }\n    } else if (pick == ST_LEAF) {\n", '< floor_n) break;\n      }\n      RL_CG_MARK("TRAV_E");\n    } else if (pick == ST_LEAF) {\n      RL_CG_MARK("LEAF_B");\n'),
    ("        state = w >> 29;\n      }\n    } else if (SPLIT_LEAF && LDS_SCENE == 4 && pick == ST_LEAF2) {",
     '        state = w >> 29;\n      }\n      RL_CG_MARK("LEAF_E");\n    } else if (SPLIT_LEAF && LDS_SCENE == 4 && pick == ST_LEAF2) {'),
    ("    } else if (pick == ST_FILL) {\n      if (state == ST_FILL) {\n        rng.top_up();\n        state = shade_state();\n      }\n",
     '    } else if (pick == ST_FILL) {\n      RL_CG_MARK("FILL_B");\n      if (state == ST_FILL) {\n        rng.top_up();\n        state = shade_state();\n      }\n      RL_CG_MARK("FILL_E");\n'),
    ("    } else if (pick == ST_GEN) {\n      bool active = false;", '    } else if (pick == ST_GEN) {\n      RL_CG_MARK("GEN_B");\n      bool active = false;'),
    (" : fast_root_word);\n        }\n      }\n", ' : fast_root_word);\n        }\n      }\n      RL_CG_MARK("GEN_E");\n'),
    ("    } else {  // ST_SHADE\n      if (state == ST_SHADE) {", '    } else {  // ST_SHADE\n      RL_CG_MARK("SHADE_B");\n      if (state == ST_SHADE) {'),
    ("        else shade(std::integral_constant<int, 0>{});\n      }\n", '        else shade(std::integral_constant<int, 0>{});\n      }\n      RL_CG_MARK("SHADE_E");\n'),
]


def makefile_flags(tree):
    """HIPCC, ARCH and CXXFLAGS as the product's Makefile states them."""
    txt = open(os.path.join(tree, CSRC, "Makefile")).read()
    get = lambda k: re.search(rf"^{k}\s*\??=\s*(.*)$", txt, re.M).group(1).strip()
    return os.environ.get("HIPCC", get("HIPCC")), get("ARCH"), get("CXXFLAGS").split()


def compile_instance(tree, name, workdir):
    """The instantiation's assembly text."""
    hipcc, arch, flags = makefile_flags(tree)
    inc = [os.path.join(tree, CSRC)]
    extra = []
    body = open(os.path.join(tree, CSRC, "rl_rtiow_wave_body.inc")).read()
    if "RL_CG_MARK" not in body:  # a tree from before the marks: a marked copy of the body shadows the tree's own
        for a, b in _OLD_BODY_MARKS:
            if body.count(a) != 1:
                raise RuntimeError(f"{tree}: cannot place the marks in this body (anchor {a[:40]!r} occurs {body.count(a)} times)")
            body = body.replace(a, b)
        shadow = os.path.join(workdir, "shadow", CSRC)  # same depth as in the tree: the headers name ../../include
        os.makedirs(shadow, exist_ok=True)
        shutil.copytree(os.path.join(tree, "include"), os.path.join(workdir, "shadow", "include"))
        for f in os.listdir(inc[0]):  # `#include "..."` looks beside the including file first: the headers move with the body
            if f.endswith((".h", ".inc")):
                shutil.copy(os.path.join(inc[0], f), shadow)
        open(os.path.join(shadow, "rl_rtiow_wave_body.inc"), "w").write(body)
        inc, extra = [shadow], [MARK_MACRO]
    src = os.path.join(workdir, name + ".hip")
    open(src, "w").write('#include <hip/hip_runtime.h>\n#include "rl_scene.h"\n#include "rl_rtiow_kernel.h"\n#include "rl_rtiow_wave.h"\n#include "rl_rtiow_coop.h"\n'
                         f"template __global__ void {INSTANCES[name]}(rl::RtiowParams);\n")
    out = os.path.join(workdir, name + ".s")
    cmd = [hipcc, f"--offload-arch={arch}", *flags, "-w", *extra, *[f"-I{d}" for d in inc], f"-I{os.path.join(tree, 'include')}", "--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout}")
    return open(out).read()


def kernel_text(asm, kernel_hint):
    """(symbol, lines of its function body, metadata dict) of the one wave kernel in the translation unit."""
    m = re.search(rf"^(_Z\w*{kernel_hint}\w*):", asm, re.M)
    sym = m.group(1)
    end = asm.index(".Lfunc_end", m.end())
    meta = {}
    entry = next(e for e in asm[asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(rf"\.name:\s+{sym}\n", e))  # its metadata entry
    for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "agpr_count"):
        mm = re.search(rf"\.{k}:\s+(\d+)", entry)
        meta[k] = int(mm.group(1)) if mm else 0
    return sym, asm[m.end():end].splitlines(), meta


class Node:
    __slots__ = ("insts", "mark", "succ", "skip", "term", "target")

    def __init__(self):
        self.insts, self.mark, self.succ, self.skip, self.term, self.target = [], None, [], None, None, None


def build_cfg(lines):
    """Basic blocks, cut again at every mark, with their successors."""
    nodes, labels = [Node()], {}
    for ln in lines:
        s = ln.strip()
        m = re.match(r"^(\.?LBB\d+_\d+):", s)
        if m:
            if nodes[-1].insts or nodes[-1].mark:
                nodes.append(Node())
            labels[m.group(1)] = len(nodes) - 1
            continue
        m = re.match(r"^; rl_cg (\w+)", s)
        if m:
            if nodes[-1].insts or nodes[-1].mark:
                nodes.append(Node())
            nodes[-1].mark = m.group(1)
            continue
        if not s or s[0] in ";." or not re.match(r"^[a-z]", s):
            continue
        op = s.split()[0]
        nodes[-1].insts.append(op)
        if op.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
            nodes[-1].term = op
            tgt = s.split()
            nodes[-1].target = tgt[1] if len(tgt) > 1 and op != "s_endpgm" else None
            nodes.append(Node())
    for i, n in enumerate(nodes):
        nxt = i + 1 if i + 1 < len(nodes) else None
        t = labels.get(n.target) if n.target else None
        if n.term is None:
            n.succ = [nxt] if nxt is not None else []
        elif n.term == "s_branch":
            n.succ = [t]
        elif n.term.startswith("s_cbranch"):
            n.succ = [nxt, t]
            n.skip = t if n.term == "s_cbranch_execz" else None  # the edge that skips a divergent region
        else:
            n.succ = []
        n.succ = [x for x in n.succ if x is not None]
    for i, n in enumerate(nodes):  # an s_cbranch_execz that is the only way out of a lane loop skips nothing: its target cannot be reached around it
        if n.skip is not None:
            seen, todo = {i}, [i + 1]
            while todo and n.skip not in seen:
                u = todo.pop()
                if u not in seen and u < len(nodes):
                    seen.add(u)
                    todo += nodes[u].succ
            if n.skip not in seen:
                n.skip = None
    return nodes


def shortest(nodes, start, goal_mark):
    """Shortest path from node `start` to the nearest node marked goal_mark other than `start` itself: (nodes walked, goal).
    Fewest skipped divergent regions first (a loop that only an s_cbranch_execz leaves has to take one), then fewest instructions."""
    SKIP = 1 << 30
    dist, prev, heap = {start: 0}, {}, [(0, start)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist.get(u, 1 << 62):
            continue
        if u != start and nodes[u].mark == goal_mark:
            path = []
            g = u
            while u != start:
                u = prev[u]
                path.append(u)
            return path[::-1], g
        for v in nodes[u].succ:
            nd = d + len(nodes[u].insts) + (SKIP if v == nodes[u].skip else 0)
            if nd < dist.get(v, 1 << 62):
                dist[v], prev[v] = nd, u
                heapq.heappush(heap, (nd, v))
    return None, None


def tally(nodes, path):
    ops = [op for i in path for op in nodes[i].insts]
    valu = [op for op in ops if op.startswith("v_")]
    return {"insts": len(ops), "valu": len(valu), "mov": sum(op.startswith(("v_mov_b", "v_accvgpr")) for op in valu),
            "lane": sum(op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")) for op in valu)}


def pick_paths(nodes):
    heads = [i for i, n in enumerate(nodes) if n.mark == "HEAD"]
    if not heads:
        raise RuntimeError("no HEAD mark in the assembly")
    out = {}
    for b in BLOCKS:
        way = ["HEAD", f"{b}_B"] + (["STEP_B", "STEP_E", "STEP_B", "STEP_E"] if b == "TRAV" else []) + [f"{b}_E", "HEAD"]
        best = None
        for h in heads:
            cur, walked, step = h, [], None
            for w in way[1:]:
                seg, g = shortest(nodes, cur, w)
                if seg is None:
                    walked = None
                    break
                if w == "STEP_E" and step is None:
                    step = tally(nodes, seg)["valu"]
                walked += seg
                cur = g
            if walked is not None:
                t = tally(nodes, walked)
                if b == "TRAV":
                    t["step"] = step
                if best is None or t["insts"] < best["insts"]:
                    best = t
        if best is not None:
            out[b] = best
    return out


ROUNDS = 4  # double rounds of ChaCha8: the trip count of the rolled loop


def pass_counts(nodes):
    """{"FULL": [valu per copy], "QUAD": [...], "quad_max": R} — empty lists for a tree without the pass marks."""
    out = {}
    for form in ("FULL", "QUAD"):
        out[form] = []
        for i, n in enumerate(nodes):
            if n.mark != f"{form}_B":
                continue
            seg, _ = shortest(nodes, i, f"{form}_E")
            if seg is None:
                continue
            out[form].append(sum(sum(op.startswith("v_") for op in nodes[u].insts) * (ROUNDS if u in nodes[u].succ else 1) for u in seg))
    if out["FULL"] and out["QUAD"]:
        out["quad_max"] = min(63, (out["FULL"][0] - 1) // out["QUAD"][0] * 16)
    return out


def report_instance(tree, name, workdir):
    asm = compile_instance(tree, name, workdir)
    _, lines, meta = kernel_text(asm, INSTANCES[name].split("::")[1].split("<")[0])
    nodes = build_cfg(lines)
    ops = [op for n in nodes for op in n.insts]
    meta.update(insts=len(ops), valu=sum(op.startswith("v_") for op in ops), mov=sum(op.startswith("v_mov_b") for op in ops),
                lane=sum(op.startswith(("v_readlane", "v_writelane")) for op in ops))
    return {"kernel": meta, "paths": pick_paths(nodes), "passes": pass_counts(nodes)}


def report(tree=ROOT, names=None):
    """{instantiation: {"kernel": register figures and whole-kernel counts, "paths": {block: pick-path counts}}}"""
    names = list(names or INSTANCES)
    with tempfile.TemporaryDirectory() as wd, concurrent.futures.ThreadPoolExecutor(max_workers=min(len(names), 8)) as ex:
        dirs = {n: os.path.join(wd, n) for n in names}
        for d in dirs.values():
            os.makedirs(d)
        return dict(zip(names, ex.map(lambda n: report_instance(tree, n, dirs[n]), names)))


def print_report(rep, base=None):
    def cell(new, old):
        return f"{new}" if old is None else f"{old}->{new}"
    for name, r in rep.items():
        b = base.get(name) if base else None
        k, kb = r["kernel"], (b["kernel"] if b else {})
        print(f"{name}: " + "  ".join(f"{lbl} {cell(k[key], kb.get(key))}" for lbl, key in (("vgpr", "vgpr_count"), ("v_spill", "vgpr_spill_count"), ("s_spill", "sgpr_spill_count"),
              ("scratch", "private_segment_fixed_size"), ("insts", "insts"), ("valu", "valu"), ("v_mov", "mov"), ("lane", "lane"))))
        for blk in BLOCKS:
            p, pb = r["paths"].get(blk), (b["paths"].get(blk) if b else None)
            if p is None:
                print(f"  {blk:5s} path not found")
                continue
            print(f"  {blk:5s} " + "  ".join(f"{key} {cell(p[key], pb.get(key) if pb else None)}" for key in ("insts", "valu", "mov", "lane") + (("step",) if blk == "TRAV" else ())))
        ps = r.get("passes") or {}
        if ps.get("FULL") or ps.get("QUAD"):
            print(f"  pass  full valu {ps.get('FULL')}  quad valu {ps.get('QUAD')}  quad_max {ps.get('quad_max')}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree", nargs="?", default=ROOT)
    ap.add_argument("--base", help="a second tree (the parent commit's checkout) whose figures are printed as the baseline")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--only", help="comma-separated instantiation names: " + ", ".join(INSTANCES))
    a = ap.parse_args()
    names = a.only.split(",") if a.only else None
    rep = report(os.path.abspath(a.tree), names)
    base = report(os.path.abspath(a.base), names) if a.base else None
    if a.json:
        print(json.dumps({"tree": rep, "base": base} if base else rep))
    else:
        print_report(rep, base)


if __name__ == "__main__":
    main()
