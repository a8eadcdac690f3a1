#!/usr/bin/env python3
"""Record tests/golden/dns/collect_parent.npz: ddpg_rollout.collect() WITHOUT a decoder on the fixed case of
tests/dns_collect_case.py, on the GPU.  Run on the commit BEFORE collect() learned the search decoder (or on any later one whose
plain path is trusted): tests/test_dns_gpu.py::test_collect_without_the_decoder_is_the_parents replays the case and compares.
CYGYM_DDPG_ROLLOUT=<path to another ddpg_rollout.py> records with that file's collect() in place of the package's (the parent
commit's file, exported with `git show`), so that the record can be made from a later working tree."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import cygym_amd.ddpg_rollout as live
    other = os.environ.get("CYGYM_DDPG_ROLLOUT")
    if other:
        spec = importlib.util.spec_from_file_location("cygym_amd._recorded_ddpg_rollout", other)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod      # (its dataclasses look their module up)
        spec.loader.exec_module(mod)
        live.collect = mod.collect
    import dns_collect_case as case
    out = case.run()
    path = os.path.join(ROOT, "tests", "golden", "dns", "collect_parent.npz")
    if len(sys.argv) > 1:
        path = sys.argv[1]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {int(out['done'].sum())} dones, reward sum {out['reward'].sum():.6f}")


if __name__ == "__main__":
    main()
