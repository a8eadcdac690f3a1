"""Build libcygym_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
from __future__ import annotations

import json
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "cygym_hip.hip")
INC = os.path.join(os.path.dirname(HERE), "include")
SO = os.path.join(HERE, "libcygym_hip.so")


def needs_build() -> bool:
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    import glob
    deps = [SRC, os.path.join(INC, "cygym_abi.h"), os.path.join(INC, "cygym_spec.h")]
    deps += [f for pat in ("*.hpp", "*.hip", "*.inc") for f in glob.glob(os.path.join(os.path.dirname(SRC), pat))]
    return any(os.path.getmtime(d) > t for d in deps)


RESOURCES = os.path.join(HERE, "build_resources.json")


def _parse_resources(text: str) -> dict:
    """kernel name -> {vgprs, sgprs, sgpr_spill, vgpr_spill, scratch, lds, occupancy} from -Rpass-analysis=kernel-resource-usage."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgprs", r"\bTotalSGPRs: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return out


INST = os.path.join(HERE, "csrc", "cg_inst.hip")
INST_ACTOR = os.path.join(HERE, "csrc", "cg_inst_actor.hip")
INST_COORD = os.path.join(HERE, "csrc", "cg_inst_coord.hip")
INST_COORD_POP = os.path.join(HERE, "csrc", "cg_inst_coord_pop.hip")
INST_COMMITTEE = os.path.join(HERE, "csrc", "cg_inst_committee.hip")
INST_DNS = os.path.join(HERE, "csrc", "cg_inst_dns.hip")
INST_MIXTURE = os.path.join(HERE, "csrc", "cg_inst_mixture.hip")
INST_COMM =os.path.join(HERE, "csrc", "cg_inst_comm.hip")
INST_COMM_POP = os.path.join(HERE, "csrc", "cg_inst_comm_pop.hip")
INST_COMM_GAT = os.path.join(HERE, "csrc", "cg_inst_comm_gat.hip")
INST_GAT_EVAL = os.path.join(HERE, "csrc", "cg_inst_gat_eval.hip")
INST_HIER = os.path.join(HERE, "csrc", "cg_inst_hier.hip")
INST_HIER_POP = os.path.join(HERE, "csrc", "cg_inst_hier_pop.hip")
INST_HMARL = os.path.join(HERE, "csrc", "cg_inst_hmarl.hip")
INST_HMARL_TRAIN = os.path.join(HERE, "csrc", "cg_inst_hmarl_train.hip")
INST_HMARL_POP = os.path.join(HERE, "csrc", "cg_inst_hmarl_pop.hip")
INST_META = os.path.join(HERE, "csrc", "cg_inst_meta.hip")
INST_META_POP = os.path.join(HERE, "csrc", "cg_inst_meta_pop.hip")
INST_META_SELECT = os.path.join(HERE, "csrc", "cg_inst_meta_select.hip")
INST_EVAL = os.path.join(HERE, "csrc", "cg_inst_eval.hip")
INST_DDPG = os.path.join(HERE, "csrc", "cg_inst_ddpg.hip")
INST_PPO = os.path.join(HERE, "csrc", "cg_inst_ppo.hip")
INST_IPPO = os.path.join(HERE, "csrc", "cg_inst_ippo.hip")
INST_NASH = os.path.join(HERE, "csrc", "cg_inst_nash.hip")
N_GROUPS = 8   # CG_INST_GROUPS of csrc/cg_device.hpp
GROUP_MT = {0: 256, 1: 256, 2: 64, 3: 64, 4: 0, 5: 0, 6: 0, 7: 0}   # device-count class each instantiation group holds


def build_to(so: str, resources: str | None = None, flags: list[str] | None = None, dev_mt: int | None = None,
             verbose: bool = False, jobs: int | None = None) -> str:
    """Compile the C-ABI unit and the instantiation units (csrc/cg_inst.hip, one per group of step_kernel variants)
    in parallel, then link `so`.  dev_mt (development): only the groups of that device-count class (0, 64 or 256),
    with -DCG_DEV_MT so that handles of the other classes fail at cygym_create."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = list(flags or []) + os.environ.get("CYGYM_BUILD_FLAGS", "").split()
    if dev_mt is not None:
        flags.append(f"-DCG_DEV_MT={dev_mt}")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + INC, "-Rpass-analysis=kernel-resource-usage"] + flags
    groups = [g for g in range(N_GROUPS) if dev_mt is None or GROUP_MT[g] == dev_mt]
    jobs = jobs or int(os.environ.get("CYGYM_BUILD_JOBS", "0")) or min(len(groups) + 1, os.cpu_count() or 4)
    with tempfile.TemporaryDirectory(prefix="cygym_build_") as tmp:
        units = [("main", base + ["-c", SRC, "-o", os.path.join(tmp, "main.o")])]
        units += [(f"inst{g}", base + [f"-DCG_INST_GROUP={g}", "-c", INST, "-o", os.path.join(tmp, f"inst{g}.o")]) for g in groups]
        if dev_mt is None or dev_mt == 256:   # the tick + actor kernels (256 devices only)
            units.append(("inst_actor", base + ["-c", INST_ACTOR, "-o", os.path.join(tmp, "inst_actor.o")]))
        units.append(("inst_coord", base + ["-c", INST_COORD, "-o", os.path.join(tmp, "inst_coord.o")]))   # the coordinate-ascent decode
        units.append(("inst_coord_pop", base + ["-c", INST_COORD_POP, "-o", os.path.join(tmp, "inst_coord_pop.o")]))   # ... for a population of critics
        units.append(("inst_committee", base + ["-c", INST_COMMITTEE, "-o", os.path.join(tmp, "inst_committee.o")]))   # the committee of DDPG experts
        units.append(("inst_dns", base + ["-c", INST_DNS, "-o", os.path.join(tmp, "inst_dns.o")]))   # the dynamic neighbourhood search
        units.append(("inst_mixture", base + ["-c", INST_MIXTURE, "-o", os.path.join(tmp, "inst_mixture.o")]))   # the mixture draw and the tiled whole-actor decode
        units.append(("inst_comm", base + ["-c", INST_COMM, "-o", os.path.join(tmp, "inst_comm.o")]))   # the per-device actor-critic decode
        units.append(("inst_comm_pop", base + ["-c", INST_COMM_POP, "-o", os.path.join(tmp, "inst_comm_pop.o")]))   # ... for a population of nets
        units.append(("inst_comm_gat", base + ["-c", INST_COMM_GAT, "-o", os.path.join(tmp, "inst_comm_gat.o")]))   # ... with its attention layers
        units.append(("inst_gat_eval", base + ["-c", INST_GAT_EVAL, "-o", os.path.join(tmp, "inst_gat_eval.o")]))   # ... and their evaluate / backward (the PPO update)
        units.append(("inst_hier", base + ["-c", INST_HIER, "-o", os.path.join(tmp, "inst_hier.o")]))   # the hierarchical (HAGS) decode
        units.append(("inst_hier_pop", base + ["-c", INST_HIER_POP, "-o", os.path.join(tmp, "inst_hier_pop.o")]))   # ... for a population of nets
        units.append(("inst_hmarl", base + ["-c", INST_HMARL, "-o", os.path.join(tmp, "inst_hmarl.o")]))   # the H-MARL decode
        units.append(("inst_hmarl_train", base + ["-c", INST_HMARL_TRAIN, "-o", os.path.join(tmp, "inst_hmarl_train.o")]))   # its training decision
        units.append(("inst_hmarl_pop", base + ["-c", INST_HMARL_POP, "-o", os.path.join(tmp, "inst_hmarl_pop.o")]))   # ... for a population of strategies
        units.append(("inst_meta", base + ["-c", INST_META, "-o", os.path.join(tmp, "inst_meta.o")]))   # the MetaDOAR decode
        units.append(("inst_meta_pop", base + ["-c", INST_META_POP, "-o", os.path.join(tmp, "inst_meta_pop.o")]))   # ... for a population of strategies
        units.append(("inst_meta_select", base + ["-c", INST_META_SELECT, "-o", os.path.join(tmp, "inst_meta_select.o")]))   # its observer's selection
        units.append(("inst_eval", base + ["-c", INST_EVAL, "-o", os.path.join(tmp, "inst_eval.o")]))   # its evaluate / backward (the PPO update)
        units.append(("inst_ddpg", base + ["-c", INST_DDPG, "-o", os.path.join(tmp, "inst_ddpg.o")]))   # the critic's tail and its backward (the DDPG update)
        units.append(("inst_ppo", base + ["-c", INST_PPO, "-o", os.path.join(tmp, "inst_ppo.o")]))   # the GAE walk and the Categorical PPO loss head (the H-MARL updates)
        units.append(("inst_ippo", base + ["-c", INST_IPPO, "-o", os.path.join(tmp, "inst_ippo.o")]))   # the advantages and the PPO head of the IPPO / MAPPO update
        units.append(("inst_nash", base + ["-c", INST_NASH, "-o", os.path.join(tmp, "inst_nash.o")]))   # the support enumeration of the restricted game, a kernel per support size

        def run(unit):
            name, cmd = unit
            if verbose:
                print(" ".join(cmd), flush=True)
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"hipcc failed on unit {name}:\n" + p.stdout[-4000:])
            return p.stdout

        with ThreadPoolExecutor(max_workers=jobs) as ex:
            logs = list(ex.map(run, units))
        objs = [u[1][-1] for u in units]
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", "-o", so] + objs   # -z defs: a kernel variant
        # declared in the C-ABI unit but missing from every instantiation group fails the build, not the first dlopen
        if verbose:
            print(" ".join(link), flush=True)
        p = subprocess.run(link, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError("link failed:\n" + p.stdout[-4000:])
    if resources:
        res = {}
        for text in logs:
            res.update(_parse_resources(text))
        with open(resources, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return so


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return SO
    return build_to(SO, RESOURCES, verbose=verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
