"""Structure of the per-tick kernels' prologue -- everything a wave issues before the kernel's only workgroup barrier -- read from
the gfx950 assembly of a cross-compile (no GPU needed).  In that phase the four waves of a SIMD run the same straight-line code
at once and the segment is bound by what it ISSUES (PERFLOG.md, round 5), so the shape of the instruction stream is the thing to
keep: one batch of scalar loads in front of one wait, addresses formed without exec-mask regions, 64-bit products formed once.

Counts of the parent of round 5 (commit ad98614), same command, as instructions (the s_barrier included) / s_load / full
lgkmcnt(0) waits / s_and_saveexec / s_mul_* before the barrier:

    step_kernel<16, 256, false, false, true>  (WIDE)     614 / 33 / 18 / 27 / 26
    step_kernel<16, 256, false, false, false>            613 / 32 / 18 / 27 / 26
    step_kernel<8, 64, false, false, false>              619 / 33 / 18 / 28 / 26
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cygym_amd", "csrc")
INC = os.path.join(ROOT, "include")

# (WPB, MT, FUSED, XE, WIDE) -> the parent's instruction count and s_mul_* count before the barrier
PARENT = {
    (16, 256, False, False, True): {"instr": 614, "s_mul": 26},
    (16, 256, False, False, False): {"instr": 613, "s_mul": 26},
    (8, 64, False, False, False): {"instr": 619, "s_mul": 26},
}
ROLLOUT = (16, 256, True, False, False)   # reported, not asserted (parent: 497 instructions)


def _targs(k):
    return ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in k)


def _mangled(k):
    b = lambda v: "Lb1E" if v else "Lb0E"
    return f"_ZN7cygym_k11step_kernelILi{k[0]}ELi{k[1]}E{b(k[2])}{b(k[3])}{b(k[4])}EEvNS_7KParamsE"


@pytest.fixture(scope="module")
def prologues(tmp_path_factory):
    """kernel key -> the instructions from the kernel's label up to and including its first s_barrier."""
    tmp = tmp_path_factory.mktemp("prologue_isa")
    keys = list(PARENT) + [ROLLOUT]
    unit = tmp / "unit.hip"
    unit.write_text('#include "cg_device.hpp"\n' + "".join(
        f"template __global__ void cygym_k::step_kernel<{_targs(k)}>(const cygym_k::KParams);\n" for k in keys))
    asm = tmp / "unit.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + INC, "-I" + CSRC,
                        str(unit), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    labels = {_mangled(k) + ":": k for k in keys}
    out, cur = {}, None
    for line in asm.read_text().splitlines():
        head = line.split(";")[0].strip()
        if head in labels:
            cur = out.setdefault(labels[head], [])
            continue
        if cur is None or not head or head.startswith(".") or head.endswith(":"):
            continue   # (directives, labels, comments)
        cur.append(head)
        if head.startswith("s_barrier"):
            cur = None
    assert set(out) == set(keys) and all(v[-1].startswith("s_barrier") for v in out.values())
    return out


def _counts(ins):
    first = lambda pred: next((i for i, s in enumerate(ins) if pred(s)), len(ins))
    gather = first(lambda s: re.match(r"global_load_dword\b", s) is not None)   # the header gather: the first plain vector load
    return {
        "instr": len(ins),
        "s_load": sum(s.startswith("s_load") for s in ins),
        "last_s_load": max((i for i, s in enumerate(ins) if s.startswith("s_load")), default=-1),
        "first_region": first(lambda s: s.startswith("s_and_saveexec") or s.startswith("s_cbranch")),
        "waits": sum(re.match(r"s_waitcnt\b.*lgkmcnt\(0\)", s) is not None for s in ins),
        "saveexec": sum(s.startswith("s_and_saveexec") for s in ins),
        "saveexec_before_gather": sum(s.startswith("s_and_saveexec") for s in ins[:gather]),
        "s_mul": sum(s.startswith("s_mul_") for s in ins),
    }


@pytest.mark.parametrize("key", list(PARENT), ids=lambda k: "step_kernel<" + _targs(k) + ">")
def test_prologue_structure(prologues, key):
    c = _counts(prologues[key])
    print(key, c)
    # every scalar load of the prologue belongs to the one batch at entry: none behind the first exec-mask region or branch,
    # hence none inside one (the parent had 14 of its 33 there)
    assert c["s_load"] > 0 and c["last_s_load"] < c["first_region"], c
    assert c["waits"] <= 8, c                              # parent: 18
    assert c["s_mul"] <= PARENT[key]["s_mul"] // 2, c      # the 64-bit products are formed once
    assert c["saveexec_before_gather"] <= 1, c             # the gather's addresses are branch-free; one region guards the load
    assert c["instr"] <= PARENT[key]["instr"] - 120, c


def test_rollout_prologue_is_no_worse(prologues):
    """The rollout kernel gathers lanes < 22 only; its prologue shares the text and must not grow (parent: 497 instructions)."""
    c = _counts(prologues[ROLLOUT])
    print(ROLLOUT, c)
    assert c["instr"] <= 497 and c["last_s_load"] < c["first_region"], c
