"""TEST-ONLY: what the CPU tests of the host planners share (test_tableplan_cpu.py, test_scanplan_cpu.py) — building a host harness
(tests/*_host.cpp with the product's compiler units, g++ only) and writing its case files (tests/plan_case.h)."""
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "pingoo_amd", "csrc")
COMPILER_UNITS = ["frontend.cpp", "pattern.cpp", "dfa.cpp", "iptrie.cpp", "filter.cpp", "residual.cpp", "compile.cpp"]
U32 = 0xFFFFFFFF


def tool(name, src, units, *extra):
    """builds tests/_build/<name> from the harness `src` and the csrc `units` on demand (one object per unit, in parallel), again when a
    source or header is newer"""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    deps = [src, os.path.join(HERE, "plan_case.h"), os.path.join(ROOT, "include", "pwaf.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".cpp", ".h", ".inc"))]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    objdir = os.path.join(BUILD, name + "_obj")
    os.makedirs(objdir, exist_ok=True)
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), *extra]
    jobs = []
    for unit in [os.path.join(CSRC, u) for u in units] + [src]:
        obj = os.path.join(objdir, os.path.basename(unit) + ".o")
        jobs.append((obj, subprocess.Popen(["g++", *flags, "-c", unit, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for obj, p in jobs:
        text, _ = p.communicate()
        assert p.returncode == 0, text[-4000:]
    subprocess.run(["g++", *extra, *[obj for obj, _ in jobs], "-o", out], check=True)
    return out


def pack_str(s):
    if s is None:
        return struct.pack("<I", U32)
    b = s.encode("utf-8", "surrogateescape") if isinstance(s, str) else bytes(s)
    return struct.pack("<I", len(b)) + b


def write_case(path, rules, routes=None, lists=None, geo=None, flags=0, opts=None, tail=b""):
    """rules [(name, expression | None, [actions])], routes [(name, expression | None)], lists {name: (type, [items])}, geo: GEOIP_DTYPE array,
    opts: (lds_table_budget, max_dfa_states, max_table_bytes) of pwaf_options, tail: what the harness reads behind the case"""
    routes, lists = routes or [], lists or {}
    n_geo = 0 if geo is None else len(geo)
    out = [b"PWAFCAS1", struct.pack("<5I", flags, len(rules), len(routes), len(lists), n_geo)]
    for name, expr, acts in rules:
        out += [pack_str(name), pack_str(expr), struct.pack("<I", len(acts)), bytes(acts)]
    for name, expr in routes:
        out += [pack_str(name), pack_str(expr)]
    for name, (typ, items) in lists.items():
        out += [pack_str(name), struct.pack("<II", typ, len(items))] + [pack_str(i) for i in items]
    if n_geo:
        out.append(np.ascontiguousarray(geo).tobytes())
    if opts:
        out.append(b"CASEOPTS" + struct.pack("<3I", *opts))
    out.append(tail)
    with open(path, "wb") as f:
        f.write(b"".join(out))
