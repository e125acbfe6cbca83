#!/usr/bin/env python
"""Memory instructions and waits of a kernel of fused.hip in issue order, read off the gfx950 assembly (needs no GPU).

    python tools/wait_chain.py [--src PATH] [--all] KERNEL [KERNEL ...]

fused.hip is compiled with the Makefile's CXXFLAGS to device assembly; for every kernel whose (mangled or demangled) name contains KERNEL
the listing shows, in the order of the text, every vector load / store / atomic, every scalar load and every s_waitcnt with the line of the
function body it stands on.  A wait also shows how many vector and scalar loads (and stores) were issued since the previous wait: a wait that
follows one or two loads is a round trip the wave makes for those alone.  Branch targets and branches are shown too (the text order is not the
execution order across them), LDS traffic only as a count per wait.  Then the kernel's VGPR count, LDS size and scratch size.
--all lists every instance that matches (default: the first, e.g. the <false> instance of a template)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mm3dgs_slam_amd", "csrc")


def makefile_flags():
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"CXXFLAGS\s*=\s*(.*)", line)
        if m:
            return m.group(1).replace("$(ARCH)", "gfx950").split()
    raise SystemExit("no CXXFLAGS in the Makefile")


def assembly(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + makefile_flags() + ["-I", CSRC, "--cuda-device-only", "-S", src, "-o", "-"], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-4000:])
    return r.stdout


def demangle(name):
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            return subprocess.check_output([tool, name], text=True).strip()
        except (OSError, subprocess.CalledProcessError):
            pass
    return name


def kind(op):
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vatomic" if "atomic" in op else "vload" if "_load" in op else "vstore" if "_store" in op else "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "sload"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier")):
        return "flow"
    return None


def kernels(text):
    """name -> (body lines, metadata dict)"""
    out, cur, name = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(("BB", ".L")):
            name, cur = m.group(1), []
            out[name] = [cur, {}]
            continue
        if cur is None:
            continue
        cur.append(line)
        m = re.match(r"^\s*;\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|TotalNumVgprs)\s*:\s*(\d+)", line)
        if m:
            out[name][1].setdefault(m.group(1), int(m.group(2)))
    return out


def listing(name, body, meta):
    print(f"== {demangle(name)}")
    n = {"vload": 0, "sload": 0, "vstore": 0, "vatomic": 0, "lds": 0}
    tot = dict(n)
    ln = 0
    for line in body:
        if re.match(r"^\s*\.(size|end_amdhsa_kernel|section)", line) or line.startswith(".Lfunc_end"):
            break
        ln += 1
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            print(f"{ln:6d}  {m.group(1)}:")
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(;.*)?$", line)
        if not m:
            continue
        op, args = m.group(1), m.group(2)
        k = kind(op)
        if k is None:
            continue
        if k == "lds":
            n["lds"] += 1
            tot["lds"] += 1
            continue
        if k == "wait":
            since = ", ".join(f"{v} {t}" for t, v in (("vector loads", n["vload"]), ("scalar loads", n["sload"]), ("vector stores", n["vstore"]),
                                                      ("atomics", n["vatomic"]), ("LDS ops", n["lds"])) if v)
            print(f"{ln:6d}      {op} {args:28s} <- since the previous wait: {since or 'nothing'}")
            n = dict.fromkeys(n, 0)
            continue
        if k in n:
            n[k] += 1
            tot[k] += 1
        print(f"{ln:6d}  {'  ' if k == 'flow' else ''}{op} {args}")
    by = {}
    for line in body:
        m = re.match(r"^\s+(global_store_\w+|global_load_\w+|s_load_\w+)\s", line)
        if m:
            by[m.group(1)] = by.get(m.group(1), 0) + 1
    print("-- totals: " + ", ".join(f"{v} {k}" for k, v in tot.items()))
    print("-- by width: " + ", ".join(f"{v} {k}" for k, v in sorted(by.items())))
    print(f"-- VGPRs {meta.get('NumVgprs', '?')} (+ {meta.get('NumAgprs', 0)} AGPRs), LDS {meta.get('LDSByteSize', '?')} bytes + the launch's dynamic bytes, "
          f"scratch {meta.get('ScratchSize', '?')} bytes, occupancy {meta.get('Occupancy', '?')} waves per SIMD")
    print()


def main():
    args = sys.argv[1:]
    src = os.path.join(CSRC, "fused.hip")
    if "--src" in args:
        i = args.index("--src")
        src = args[i + 1]
        del args[i:i + 2]
    every = "--all" in args
    args = [a for a in args if a != "--all"]
    if not args:
        raise SystemExit(__doc__)
    ks = kernels(assembly(src))
    for want in args:
        hits = [k for k in ks if want in k or want in demangle(k)]
        if not hits:
            raise SystemExit(f"no kernel matches {want!r}")
        for k in (hits if every else hits[:1]):
            listing(k, *ks[k])


if __name__ == "__main__":
    main()
