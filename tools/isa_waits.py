#!/usr/bin/env python3
"""How the flight kernels wait for their model-table reads, read off the assembly (no GPU involved).

Compiles flybody_amd/csrc/fly_env.hip to gfx950 assembly with the library's own flags (build._common_flags() plus the per-source
flags) and prints, for flight_step_kernel<6|12>, flight_collide_a and flight_collide_b:

  s_load                 scalar memory loads
  s_load_dwordx2         ... of them 64-bit: a pointer fetched from a struct (or a kernel argument)
  s_wait_groups / _near  s_waitcnt lgkmcnt(0) with a scalar load outstanding / with the newest such load at most NEAR_WAIT
                         instructions before the wait (an exposed scalar-cache round trip)
  g_sbase / _near        global memory operations whose SGPR base pair was written by an s_load / at most NEAR_BASE instructions
                         after that s_load (the two-level chain: fetch the table's pointer, then read the table)
  v_load                 vector memory loads (global_load, flat_load, scratch_load excluded)
  v_wait_groups / _near  s_waitcnt vmcnt(n) with a vector load outstanding / with the newest at most NEAR_WAIT instructions before
  v_chained              vector loads of 64 bits or more whose result is used only to address other vector loads, straight or
                         through address arithmetic: a table pointer fetched by a vector load

Register tracking is linear over the instruction stream of a function (branches are not followed): good for counting, not a proof.

  python tools/isa_waits.py                     table for the working tree
  python tools/isa_waits.py --json              the same as one JSON object
  python tools/isa_waits.py --src DIR           csrc directory of another checkout (e.g. the parent commit)
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEAR_WAIT = 6
NEAR_BASE = 12
ADDR_ARITH = re.compile(r"v_(add|addc|lshl_add|lshlrev|mad_u64|mov|lshl_or|add3|ashrrev)")  # what forms an address from a pointer and an index
FUNCS = ("flight_step_kernelILi6E", "flight_step_kernelILi12E", "flight_collide_aILi6E", "flight_collide_aILi12E", "flight_collide_bILi6E",
         "flight_collide_bILi12E")


def assembly(csrc: str) -> str:
    from flybody_amd import build

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "fly_env.s")
        cmd = build._common_flags() + build.PER_SOURCE_FLAGS.get("fly_env.hip", []) + ["--cuda-device-only", "-S", os.path.join(csrc, "fly_env.hip"), "-o", out]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def functions(text: str) -> dict:
    """{mangled name: [instruction lines]} of the functions in FUNCS."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), []) if any(k in m.group(1) for k in FUNCS) else None
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(s)
    return out


def _regs(tok: str, kind: str) -> list:
    """Register numbers named by an operand like s[4:5], v12, s7 of the given kind ('s' or 'v')."""
    m = re.fullmatch(kind + r"\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(kind + r"(\d+)", tok)
    return [int(m.group(1))] if m else []


def _operands(ins: str) -> list:
    parts = ins.split(None, 1)
    return [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []


def measure(lines: list) -> dict:
    r = dict(s_load=0, s_load_dwordx2=0, s_wait_groups=0, s_wait_near=0, g_sbase=0, g_sbase_near=0, v_load=0, v_wait_groups=0, v_wait_near=0, v_chained=0)
    sdef = {}          # SGPR -> index of the s_load that wrote it last (absent: written by something else)
    last_s = last_v = None
    s_out = v_out = False
    for i, ins in enumerate(lines):
        op = ins.split()[0]
        ops = _operands(ins)
        if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            r["s_load"] += 1
            r["s_load_dwordx2"] += op == "s_load_dwordx2"
            for k in _regs(ops[0], "s"):
                sdef[k] = i
            last_s, s_out = i, True
            continue
        is_vmem = op.startswith("global_") or op.startswith("flat_")
        if is_vmem:
            for t in ops:
                if t.split()[0].startswith("s["):
                    base = _regs(t.split()[0], "s")
                    if base and all(k in sdef for k in base):
                        r["g_sbase"] += 1
                        r["g_sbase_near"] += i - max(sdef[k] for k in base) <= NEAR_BASE
            if "_load_" in op:
                r["v_load"] += 1
                last_v, v_out = i, True
            continue
        if op == "s_waitcnt":
            if "lgkmcnt(0)" in ins and s_out:
                r["s_wait_groups"] += 1
                r["s_wait_near"] += i - last_s <= NEAR_WAIT
                s_out = False
            if "vmcnt(" in ins and v_out:
                r["v_wait_groups"] += 1
                r["v_wait_near"] += i - last_v <= NEAR_WAIT
                if "vmcnt(0)" in ins:
                    v_out = False
            continue
        if ops and op.startswith("s_"):  # any other scalar write ends the s_load's ownership of the register
            for k in _regs(ops[0], "s"):
                sdef.pop(k, None)
    # vector loads of 64 bits or more whose result only ever addresses other vector loads, straight or through address arithmetic
    vreg = lambda t: {k for tok in re.findall(r"v\[\d+:\d+\]|v\d+", t) for k in _regs(tok, "v")}
    for i, ins in enumerate(lines):
        op = ins.split()[0]
        if not ((op.startswith("global_load_") or op.startswith("flat_load_")) and op.endswith(("dwordx2", "dwordx3", "dwordx4"))):
            continue
        taint = set(vreg(_operands(ins)[0]))
        as_addr = other = 0
        for j in range(i + 1, len(lines)):
            if not taint:
                break
            o2, t2 = lines[j].split()[0], _operands(lines[j])
            if not t2:
                continue
            vm = o2.startswith(("global_", "flat_", "scratch_", "buffer_"))
            if vm and "_load_" in o2:
                if vreg(t2[1]) & taint:
                    as_addr += 1
                taint -= vreg(t2[0])
            elif vm or o2.startswith("ds_write") or o2.startswith("ds_bpermute"):  # stores, atomics: every operand is a read
                other += any(vreg(t) & taint for t in t2)
            else:
                reads = any(vreg(t) & taint for t in t2[1:])
                if reads and ADDR_ARITH.match(o2):
                    taint |= vreg(t2[0])
                else:
                    other += reads
                    if not o2.startswith("v_cmp"):
                        taint -= vreg(t2[0])
        r["v_chained"] += as_addr > 0 and other == 0
    return r


def report(csrc: str) -> dict:
    return {name: measure(lines) for name, lines in sorted(functions(assembly(csrc)).items())}


def short(name: str) -> str:
    m = re.search(r"(flight_\w+?)ILi(\d+)E", name)
    return f"{m.group(1)}<{m.group(2)}>" if m else name


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(ROOT, "flybody_amd", "csrc"))
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rep = report(a.src)
    if a.json:
        print(json.dumps({short(k): v for k, v in rep.items()}))
        return
    cols = list(next(iter(rep.values())).keys())
    print(f"near wait: {NEAR_WAIT} instructions, near base: {NEAR_BASE} instructions")
    print(f"{'function':28s}" + "".join(f"{c:>16s}" for c in cols))
    for k, v in rep.items():
        print(f"{short(k):28s}" + "".join(f"{v[c]:16d}" for c in cols))


if __name__ == "__main__":
    main()
