#!/usr/bin/env python3
"""kernel_diff.py OLD_TREE NEW_TREE [--prof] — are the gfx950 kernels of two trees the same code?

Compiles every pingoo_amd/csrc/*.hip of both trees for gfx950, device only, to assembly with the compiler's resource report, and compares
kernel by kernel (by mangled name, whatever unit a kernel lives in): the normalised assembly — the kernel's own and that of the out-of-line
device functions it calls — and the resource table. What depends on the unit and not on the code is normalised away: basic-block and
function label numbers, .file / .loc / .ident lines, comments, the compilation-unit id. Exits 1 on any difference. No GPU needed.
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage"]
KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def compile_unit(tree, src, prof):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        cmd = [os.environ.get("HIPCC", "hipcc"), *FLAGS, "-I", os.path.join(tree, "include"), *(["-DPWAF_PROFILING"] if prof else []), src, "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"{src}:\n{r.stderr}")
        return os.path.basename(src), open(out).read(), r.stderr


def normalise(line):
    line = re.sub(r"\s*;.*$", "", line.rstrip())
    if not line.strip() or re.match(r"\s*\.(file|loc|ident|cfi_\w+)\b", line):
        return None
    line = re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+(_(\d+))?", lambda m: f".L{m.group(1)}_{m.group(3) or ''}", line)
    return re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)


def functions(asm):
    """symbol -> (normalised lines, is a kernel), for every function of one unit's assembly."""
    out, name, body = {}, None, []
    for line in asm.split("\n"):
        m = re.match(r"(\S+):\s*; @(\S+)$", line)
        if m and m.group(1) == m.group(2):
            name, body = m.group(1), []
        if name is None:
            continue
        n = normalise(line)
        if n is not None:
            body.append(n)
        if re.match(r"\.Lfunc_end\d+:", line):
            out[name] = (body, any(l.lstrip().startswith(".amdhsa_kernel") for l in body))
            name = None
    return out


def resources(remarks):
    """function name -> {resource: value}, from the -Rpass-analysis=kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def kernels_of(tree, prof):
    """kernel symbol -> (unit, lines of the kernel and of its out-of-line callees, resource table)."""
    srcs = sorted(glob.glob(os.path.join(tree, "pingoo_amd", "csrc", "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1)) as pool:
        units = list(pool.map(lambda s: compile_unit(tree, s, prof), srcs))
    out = {}
    for unit, asm, remarks in units:
        fns, res = functions(asm), resources(remarks)
        for sym, (body, is_kernel) in fns.items():
            if not is_kernel:
                continue
            lines, seen, todo = [], set(), [sym]
            while todo:  # the kernel, then what it calls, depth first in order of first mention
                f = todo.pop()
                if f in seen:
                    continue
                seen.add(f)
                lines += [f"<{f}>"] + fns[f][0]
                text = "\n".join(fns[f][0])
                todo += sorted((c for c in fns if c not in seen and not fns[c][1] and re.search(re.escape(c) + r"\b", text)), reverse=True)
            out[sym] = (unit, lines, {k: res.get(sym, {}).get(k, "?") for k in KEYS})
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--prof"]
    if len(args) != 2:
        sys.exit(__doc__)
    prof = "--prof" in sys.argv
    old, new = kernels_of(args[0], prof), kernels_of(args[1], prof)
    print(f"# kernel_diff{' --prof' if prof else ''}: {len(old)} kernels in OLD, {len(new)} in NEW; per kernel: unit(s), {', '.join(KEYS)}")
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            print(f"ONLY IN {'OLD' if sym in old else 'NEW'}  {sym}  [{(old.get(sym) or new.get(sym))[0]}]")
            bad += 1
            continue
        (ou, ol, ores), (nu, nl, nres) = old[sym], new[sym]
        where = ou if ou == nu else f"{ou} -> {nu}"
        table = " ".join(str(nres[k]) if ores[k] == nres[k] else f"{ores[k]}->{nres[k]}" for k in KEYS)
        same = ol == nl and ores == nres
        print(f"{'identical' if same else 'DIFFERENT'}  {sym}  [{where}]  {len(nl)} lines  {table}")
        if not same:
            bad += 1
            first = next((i for i, (a, b) in enumerate(zip(ol, nl)) if a != b), min(len(ol), len(nl)))
            for i in range(first, min(first + 5, max(len(ol), len(nl)))):
                print(f"    {i}: - {ol[i] if i < len(ol) else ''}\n    {i}: + {nl[i] if i < len(nl) else ''}")
    print(f"# {len(set(old) & set(new)) - sum(1 for s in set(old) & set(new) if old[s][1:] != new[s][1:])} identical, {bad} different or missing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
