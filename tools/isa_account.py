#!/usr/bin/env python3
"""VALU instruction accounting of one row kernel, from the compiler's assembly (no GPU needed).

Builds a one-kernel translation unit for gfx950 in a temporary directory (hipcc -O3 --cuda-device-only -S -gline-tables-only),
splits the kernel's assembly into regions -- the phase function an instruction was inlined from, and the loop it sits in --
and prints, per region, how many VALU instructions there are by broad class:

    fp64    double-precision arithmetic (fma / mul / add / rcp / rsq / sqrt / div helpers / ldexp ..., DPP forms included)
    select  v_cndmask
    move    v_mov / v_accvgpr without a lane pattern
    xlane   DPP moves, v_readlane / v_writelane / v_readfirstlane / v_permlane
    int     everything else that starts with v_ (integer, compare, conversions, 32-bit float)

once as the static count and once weighted by loop trip counts.  Trip counts are ASSUMED, not measured: a loop is named
`function@depth` (depth counts the loops of that same function around it, 1 = outermost) and gets the count given with
--trips, the built-in default for N = 200 correspondences, or 1.  Out-of-line device functions are weighted by --calls.
Classification is by mnemonic prefix only.

    python tools/isa_account.py                       # k_linear_tft_pose_rows<false, false>
    python tools/isa_account.py --kernel f            # k_linear_f_pose_rows
    python tools/isa_account.py --trips rows_votes@2=7 --out profiles/isa_account_tft.txt
    python tools/isa_account.py --blocks                # the kernel's basic blocks one by one, in program order

The weighted table multiplies every block of a loop by the loop's trip count, taken or not (the second-candidate blocks of the vote loop
are never taken at N = 200): it cannot show the executed path.  --blocks lists, per basic block, the VALU count by class, the SALU count,
whether the block ends in a back edge, and the source lines most of its VALU instructions were inlined from.
"""
import argparse
import bisect
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")

KERNELS = {
    "tft": ("tft_rows_kernel.h", "template __global__ void tff::k_linear_tft_pose_rows<false, false>(const tff::LinearTftArgs);",
            "k_linear_tft_pose_rows"),
    "f": ("f_rows_kernel.h", "namespace tff { auto* isa_account_keep = &k_linear_f_pose_rows; }", "k_linear_f_pose_rows"),
}
# loop trip counts at N = 200 (13 trips of 16 correspondences); the eigen-solver counts are typical values of the debug counters
DEFAULT_TRIPS = {
    "rows_centroids@1": 3,             # whole groups of 64 correspondences (the tail group is straight-line code)
    "rows_distances_moments@1": 13,    # two half-bodies of 8 correspondences per row and trip
    "rows_linear_tft_middle@1": 8,     # Gp build: 120 entries over 16 lanes
    "rows_min_eigvec@1": 5,            # inverse iterations (two solves: 27 x 27 and 15 x 15)
    "rows_votes@1": 1,                 # sweeps
    "rows_votes@2": 13,                # trips
    "rows_votes@3": 2,                 # the two essential matrices (when the loop stays rolled)
    "rows_tri_pass@1": 13,
    "rows_distances_moments_f@1": 13,  # LinearF: one correspondence per lane and trip
    "rows_begin@1": 13,
}
DEFAULT_CALLS = {"epipoles_from_tensor": 2}
CLASSES = ("fp64", "select", "move", "xlane", "int")
FP64_PREFIXES = ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "v_rcp_f64", "v_rsq_f64", "v_sqrt_f64", "v_div_", "v_ldexp_f64",
                 "v_frexp_", "v_min_f64", "v_max_f64", "v_trig_preop_f64", "v_fract_f64", "v_floor_f64", "v_rndne_f64", "v_trunc_f64",
                 "v_ceil_f64", "v_pk_")
XLANE_PREFIXES = ("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane")


def classify(mnemonic, operands):
    if not mnemonic.startswith("v_"):
        return None
    lane_pattern = "_dpp" in mnemonic or "row_" in operands or "quad_perm" in operands
    if mnemonic.startswith(FP64_PREFIXES) and mnemonic.endswith(("f64", "f64_dpp", "f64_e32", "f64_e64")):
        return "fp64"
    if mnemonic.startswith(XLANE_PREFIXES) or (lane_pattern and mnemonic.startswith("v_mov")):
        return "xlane"
    if mnemonic.startswith("v_cndmask"):
        return "select"
    if mnemonic.startswith(("v_mov", "v_accvgpr")):
        return "move"
    return "int"


class FunctionIndex:
    """source line -> name of the function whose definition starts last before it"""
    START = re.compile(r"^(?:template\s*<.*>\s*)?(?:__device__|__global__|__host__|static|inline)\b[^;]*$")
    CALL = re.compile(r"\b([A-Za-z_]\w*)\s*\(")
    NOT_NAMES = ("__launch_bounds__", "__attribute__", "noinline", "if", "for", "while", "sizeof", "alignas")

    def __init__(self):
        self.files = {}

    def lookup(self, path, line):
        if path not in self.files:
            starts, names = [], []
            full = path if os.path.isabs(path) else os.path.join(CSRC, os.path.basename(path))
            try:
                with open(full) as f:
                    for n, text in enumerate(f, 1):
                        if not self.START.match(text):
                            continue
                        head = text.split("{", 1)[0]
                        name = next((c for c in self.CALL.findall(head) if c not in self.NOT_NAMES), None)
                        if name:
                            starts.append(n); names.append(name)
            except OSError:
                pass
            self.files[path] = (starts, names)
        starts, names = self.files[path]
        k = bisect.bisect_right(starts, line) - 1
        return names[k] if k >= 0 else os.path.basename(path)


def build_asm(kernel, workdir):
    header, inst, _ = KERNELS[kernel]
    src = os.path.join(workdir, "one_kernel.hip")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "%s"\n%s\n' % (header, inst))
    out = os.path.join(workdir, "one_kernel.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + CSRC, "--cuda-device-only", "-S", "-gline-tables-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", out, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise SystemExit("compilation failed")
    usage, mine = [], False
    ours = re.compile(r"\d+%s[EI]" % KERNELS[kernel][2])
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            mine = bool(ours.search(m.group(2)))
        if m and mine:
            usage.append((m.group(1), m.group(2)))
    with open(out) as f:
        return f.read().splitlines(), usage


FRAME = re.compile(r"([^\s\[\]@;]+):(\d+):\d+")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\s*(.*?)(?:;.*)?$")
# functions that are accounted under their own name wherever they were inlined from
LEAVES = ("gram_row27", "frame_of", "vote_one", "dlt_from_vote", "svd3", "mat3_inv")


def split_functions(lines):
    """[(symbol, [lines])] of every function body in the assembly"""
    out, cur, name = [], None, None
    for text in lines:
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s", text + " ")
        if m and cur is None and not text.startswith("."):
            name, cur = m.group(1), []
        elif text.startswith(".Lfunc_end") and cur is not None:
            out.append((name, cur)); cur = None
        elif cur is not None:
            cur.append(text)
    return out


BLOCK = re.compile(r"^(?:\.LBB(\d+_\d+):|; %bb\.\d+:)")
IN_LOOP = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")
IS_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
CHILD = re.compile(r"Child Loop BB(\d+_\d+) Depth (\d+)")
PARENT = re.compile(r"Parent Loop BB(\d+_\d+) Depth=(\d+)")


def account(body, findex, depth_frames):
    """[(phase, loop names outermost first, class)] of every VALU instruction in one function body.
    Loops are the compiler's own: every basic block's comment names the innermost loop it belongs to."""
    rows = []                # (class, frames, innermost loop header or None)
    parent = {}              # loop header -> enclosing loop header
    frames, loop, label, stack = [], None, None, []
    for text in body:
        m = BLOCK.match(text)
        if m:
            label = m.group(1)
            loop = None
            stack = []
        if m or text.startswith("      ") and text.lstrip().startswith(";"):      # a block's comment and its continuation lines
            mi, mh = IN_LOOP.search(text), IS_HEADER.search(text)
            if mi:
                loop = mi.group(1)
            for mp in PARENT.finditer(text):
                stack = stack[:int(mp.group(2)) - 1] + [mp.group(1)]
            if mh and label:
                loop = label
                d = int(mh.group(1))
                if d > 1 and len(stack) >= d - 1:
                    parent[label] = stack[d - 2]
                stack = stack[:d - 1] + [label]
            mc = CHILD.search(text)
            if mc:
                d = int(mc.group(2))
                if len(stack) >= d - 1 and d > 1:
                    parent[mc.group(1)] = stack[d - 2]
                stack = stack[:d - 1] + [mc.group(1)]
            if m or mi or mh or mc or PARENT.search(text):
                continue
        if text.lstrip().startswith(".loc"):
            here = [(f, int(l)) for f, l in FRAME.findall(text.split(";", 1)[1]) if int(l) > 0] if ";" in text else []
            frames = here or frames                      # (line 0: the compiler kept no location; the instruction stays with its neighbours)
            continue
        m = INSTR.match(text)
        if m and not m.group(1).startswith("."):
            rows.append((classify(m.group(1), m.group(2)), frames, loop))

    def names(frs):          # functions from the kernel inwards
        return [findex.lookup(f, l) for f, l in reversed(frs)]

    # a loop is named after the deepest function that at least 60 % of its own instructions (nested loops aside) were inlined from
    own = collections.defaultdict(list)
    for cls, frs, lp in rows:
        if lp is not None and frs:
            own[lp].append(names(frs))
    loop_name = {}
    for lp, chains in own.items():
        name, d = "?", 0
        while True:
            votes = collections.Counter(c[d] for c in chains if len(c) > d)
            if not votes:
                break
            best, n = votes.most_common(1)[0]
            if n < 0.6 * len(chains):
                break
            name, d = best, d + 1
        loop_name[lp] = name
    result = []
    for cls, frs, lp in rows:
        if cls is None:
            continue
        ns = names(frs)
        phase = ns[min(depth_frames, len(ns) - 1)] if ns else "?"
        for leaf in LEAVES:
            if leaf in ns:
                phase = leaf
        around = []
        while lp is not None:
            around.insert(0, lp)
            lp = parent.get(lp)
        seen = collections.Counter()
        tags = []
        for l in around:
            fn = loop_name.get(l, "?")
            seen[fn] += 1
            tags.append("%s@%d" % (fn, seen[fn]))
        result.append((phase, tuple(tags), cls))
    return result


BRANCH = re.compile(r"^s_cbranch_\w+|^s_branch$")


def blocks(body):
    """[(label, Counter of classes + 'salu', ends in a back edge, Counter of innermost source lines of the VALU instructions)] in program order"""
    out, seen = [], set()
    label, frames = "entry", []
    cur = [label, collections.Counter(), False, collections.Counter()]
    for text in body:
        m = BLOCK.match(text)
        if m:
            if sum(cur[1].values()):
                out.append(tuple(cur))
            seen.add(cur[0])
            label = "BB" + m.group(1) if m.group(1) else text.split("%", 1)[1].split(":")[0]
            cur = [label, collections.Counter(), False, collections.Counter()]
            continue
        if text.lstrip().startswith(".loc"):
            here = [(f, int(l)) for f, l in FRAME.findall(text.split(";", 1)[1]) if int(l) > 0] if ";" in text else []
            frames = here or frames
            continue
        m = INSTR.match(text)
        if not m or m.group(1).startswith("."):
            continue
        cls = classify(m.group(1), m.group(2))
        if cls is not None:
            cur[1][cls] += 1
            if frames:
                cur[3]["%s:%d" % (os.path.basename(frames[0][0]), frames[0][1])] += 1
        elif m.group(1).startswith("s_"):
            cur[1]["salu"] += 1
            if BRANCH.match(m.group(1)):
                target = m.group(2).strip().lstrip(".L")
                cur[2] = cur[2] or target in seen or target == cur[0]
    if sum(cur[1].values()):
        out.append(tuple(cur))
    return out


def blocks_report(lines, kernel, usage):
    ours = re.compile(r"\d+%s[EI]" % KERNELS[kernel][2])
    out = ["kernel %s, basic blocks in program order: VALU instructions by class, SALU instructions, back edge, top source lines" % KERNELS[kernel][2]]
    for k, v in usage:
        out.append("  %s: %s" % (k, v))
    for symbol, body in split_functions(lines):
        if not ours.search(symbol) and re.search(r"\d+k_\w+", symbol):
            continue
        out.append("")
        out.append("function %s" % symbol)
        out.append("%-12s" % "block" + "".join("%8s" % c for c in CLASSES) + "%8s %6s %6s %5s  %s" % ("VALU", "fp64%", "SALU", "back", "top source lines (VALU instructions)"))
        total = collections.Counter()
        for label, c, back, where in blocks(body):
            n = sum(c[x] for x in CLASSES)
            total.update(c)
            out.append("%-12s" % label + "".join("%8d" % c[x] for x in CLASSES) + "%8d %6.1f %6d %5s  %s"
                       % (n, 100.0 * c["fp64"] / n if n else 0.0, c["salu"], "yes" if back else "", " ".join("%s(%d)" % kv for kv in where.most_common(4))))
        n = sum(total[x] for x in CLASSES)
        out.append("%-12s" % "TOTAL" + "".join("%8d" % total[x] for x in CLASSES) + "%8d %6.1f %6d" % (n, 100.0 * total["fp64"] / n if n else 0.0, total["salu"]))
    return "\n".join(out) + "\n"


def main():
    global CSRC
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", choices=sorted(KERNELS), default="tft")
    ap.add_argument("--trips", action="append", default=[], metavar="FUNC@DEPTH=COUNT")
    ap.add_argument("--calls", action="append", default=[], metavar="FUNC=COUNT", help="calls of an out-of-line device function per kernel pass")
    ap.add_argument("--depth", type=int, default=1, help="inlining depth below the kernel that names a phase (default 1)")
    ap.add_argument("--csrc", default=CSRC, help="kernel sources to compile and to name functions from (default: this tree's; another checkout's for a comparison)")
    ap.add_argument("--asm", help="account an existing assembly file instead of compiling (it must come from the sources under --csrc)")
    ap.add_argument("--blocks", action="store_true", help="list the basic blocks one by one instead of the two region tables")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    CSRC = os.path.abspath(args.csrc)
    trips = dict(DEFAULT_TRIPS)
    for t in args.trips:
        k, v = t.split("=")
        trips[k] = float(v)
    calls = dict(DEFAULT_CALLS)
    for t in args.calls:
        k, v = t.split("=")
        calls[k] = float(v)
    if args.asm:
        with open(args.asm) as f:
            lines, usage = f.read().splitlines(), []
    else:
        with tempfile.TemporaryDirectory() as d:
            lines, usage = build_asm(args.kernel, d)
    if args.blocks:
        text = blocks_report(lines, args.kernel, usage)
        sys.stdout.write(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    findex = FunctionIndex()
    table = collections.OrderedDict()
    assumed = set()
    ours = re.compile(r"\d+%s[EI]" % KERNELS[args.kernel][2])          # the mangled name, not a longer one that starts with it
    for symbol, body in split_functions(lines):
        is_kernel = bool(ours.search(symbol))
        if not is_kernel and re.search(r"\d+k_\w+", symbol):
            continue                                                    # another kernel of the same header
        scale = 1.0
        fname = KERNELS[args.kernel][2]
        if not is_kernel:
            fname = next((n for n in calls if n in symbol), symbol)
            scale = calls.get(fname, 1.0)
        for phase, tags, cls in account(body, findex, args.depth if is_kernel else 0):
            w = scale
            for t in tags:
                if t not in trips:
                    assumed.add(t)
                w *= trips.get(t, 1.0)
            inner = tags[-1] if tags else "-"
            key = (phase if is_kernel else fname + " (out of line)", inner)
            row = table.setdefault(key, {"static": collections.Counter(), "weighted": collections.Counter()})
            row["static"][cls] += 1
            row["weighted"][cls] += w
    out = []
    out.append("kernel %s, VALU instructions per wavefront (four triplets) by region and class" % KERNELS[args.kernel][2])
    for k, v in usage:
        out.append("  %s: %s" % (k, v))
    out.append("trip counts (assumed): " + ", ".join("%s=%g" % kv for kv in sorted(trips.items())))
    out.append("calls (assumed): " + ", ".join("%s=%g" % kv for kv in sorted(calls.items())))
    if assumed:
        out.append("loops counted once (no trip count given): " + ", ".join(sorted(assumed)))
    for mode in ("static", "weighted"):
        out.append("")
        out.append("%-8s %-34s %-30s" % (mode, "phase", "innermost loop") + "".join("%9s" % c for c in CLASSES) + "%10s %6s" % ("VALU", "fp64%"))
        total = collections.Counter()
        for (phase, inner), row in sorted(table.items(), key=lambda kv: -sum(kv[1]["weighted"].values())):
            c = row[mode]
            n = sum(c.values())
            total.update(c)
            out.append("%-8s %-34s %-30s" % ("", phase[:34], inner[:30]) + "".join("%9.0f" % c[x] for x in CLASSES)
                       + "%10.0f %6.1f" % (n, 100.0 * c["fp64"] / n if n else 0.0))
        n = sum(total.values())
        out.append("%-8s %-34s %-30s" % ("", "TOTAL", "") + "".join("%9.0f" % total[x] for x in CLASSES)
                   + "%10.0f %6.1f" % (n, 100.0 * total["fp64"] / n if n else 0.0))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
