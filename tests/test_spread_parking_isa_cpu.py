"""What the compile-time spread (csrc/cg_attacker.hpp, attacker_spread_ct) parks in the lanes of a spill VGPR, read from the
gfx950 assembly of a cross-compile (no GPU needed).  The spread runs while all sixteen waves of a CU are alive, where a segment
costs what it ISSUES (PERFLOG.md, rounds 4 and 5), and it is the chain of the env every attacker launch waits for: a uniform value
hoisted out of its loops is a v_writelane (with hazard no-ops) at its top and v_readlane's all through the sweeps, the counts and
the ring.  Counted per kernel: `.sgpr_spill_count` of the metadata, and v_writelane / v_readlane between the first `s_setprio 3`
(the spread's call) and the next `s_setprio 0`.

The parent of round 12 (commit 4800242), same command: spill slots / v_writelane / v_readlane

    step_kernel<16, 256, false, false, true>  (WIDE)     68 / 57 / 141
    step_kernel<16, 256, false, false, false>            73 / 54 / 152
    step_kernel<8, 64, false, false, false>              18 / 16 /  45
    step_kernel<16, 256, true, false, false> (rollout)  124 / 43 / 169

The bounds: the WIDE kernel at most 42 / 25 / 85 (what making `n_src` opaque at four places reached; the finished text is well
below, and a toolchain that moves a few slots does not break the test), the other two per-tick kernels strictly below the parent
in every figure, the rollout kernel not above it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cygym_amd", "csrc")
INC = os.path.join(ROOT, "include")

WIDE = (16, 256, False, False, True)
LEAN256 = (16, 256, False, False, False)
LEAN64 = (8, 64, False, False, False)
ROLLOUT = (16, 256, True, False, False)
# (WPB, MT, FUSED, XE, WIDE) -> the parent's figures
PARENT = {
    WIDE: {"sgpr_spill": 68, "writelane": 57, "readlane": 141},
    LEAN256: {"sgpr_spill": 73, "writelane": 54, "readlane": 152},
    LEAN64: {"sgpr_spill": 18, "writelane": 16, "readlane": 45},
    ROLLOUT: {"sgpr_spill": 124, "writelane": 43, "readlane": 169},
}
WIDE_BOUND = {"sgpr_spill": 42, "writelane": 25, "readlane": 85}


def _targs(k):
    return ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in k)


def _mangled(k):
    b = lambda v: "Lb1E" if v else "Lb0E"
    return f"_ZN7cygym_k11step_kernelILi{k[0]}ELi{k[1]}E{b(k[2])}{b(k[3])}{b(k[4])}EEvNS_7KParamsE"


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    """kernel key -> {"sgpr_spill", "vgprs", "vgpr_spill", "region", "writelane", "readlane"}."""
    tmp = tmp_path_factory.mktemp("spread_parking_isa")
    keys = list(PARENT)
    unit = tmp / "unit.hip"
    unit.write_text('#include "cg_device.hpp"\n' + "".join(
        f"template __global__ void cygym_k::step_kernel<{_targs(k)}>(const cygym_k::KParams);\n" for k in keys))
    asm = tmp / "unit.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + INC, "-I" + CSRC,
                        str(unit), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    text = asm.read_text()
    labels = {_mangled(k) + ":": k for k in keys}
    body, cur = {}, None
    for line in text.splitlines():
        head = line.split(";")[0].strip()
        if head in labels:
            cur = body.setdefault(labels[head], [])
            continue
        if head.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not head or head.startswith(".") or head.endswith(":"):
            continue   # (directives, labels, comments)
        cur.append(head)
    assert set(body) == set(keys)
    # the metadata: one entry per kernel, its fields in alphabetical order from .agpr_count on
    meta = {}
    for ent in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", ent).group(1)
        meta[name] = {f: int(re.search(r"\." + f + r":\s+(\d+)", ent).group(1)) for f in ("sgpr_spill_count", "vgpr_count", "vgpr_spill_count")}
    out = {}
    for k in keys:
        ins = body[k]
        a = next(i for i, s in enumerate(ins) if s.startswith("s_setprio 3"))
        b = next(i for i in range(a, len(ins)) if ins[i].startswith("s_setprio 0"))
        reg = ins[a:b]
        m = meta[_mangled(k)]
        out[k] = {"sgpr_spill": m["sgpr_spill_count"], "vgprs": m["vgpr_count"], "vgpr_spill": m["vgpr_spill_count"], "region": len(reg),
                  "writelane": sum(s.startswith("v_writelane") for s in reg), "readlane": sum(s.startswith("v_readlane") for s in reg)}
    return out


def test_wide_kernel_parks_no_more_than_the_bound(figures):
    c = figures[WIDE]
    print("step_kernel<" + _targs(WIDE) + ">", c)
    for f, bound in WIDE_BOUND.items():
        assert c[f] <= bound, (f, c)
    assert c["vgpr_spill"] == 0 and c["vgprs"] <= 96, c


@pytest.mark.parametrize("key", [LEAN256, LEAN64], ids=lambda k: "step_kernel<" + _targs(k) + ">")
def test_lean_per_tick_kernels_park_less_than_the_parent(figures, key):
    c = figures[key]
    print("step_kernel<" + _targs(key) + ">", c)
    for f, parent in PARENT[key].items():
        assert c[f] < parent, (f, c)
    assert c["vgpr_spill"] == 0, c


def test_rollout_kernel_parks_no_more_than_the_parent(figures):
    c = figures[ROLLOUT]
    print("step_kernel<" + _targs(ROLLOUT) + ">", c)
    for f, parent in PARENT[ROLLOUT].items():
        assert c[f] <= parent, (f, c)
    assert c["vgpr_spill"] == 0, c
