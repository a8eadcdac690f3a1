"""The spread's sweeps reach the same fix point whichever way the blocks of sources take turns (cygym_amd/csrc/cg_attacker.hpp,
attacker_spread_ct: the serial verification sweeps, and the merged one in which the losers of blocks 0 and 1 rescan together and see
each other's takes a sweep later).

tests/spread_fixpoint_probe.cpp models the takes on the host -- the lowest source id wins a target, a loser rescans behind its pick --
and runs both orders to their fix points on random and adversarial small instances: 2 .. 130 sources, rows of 1 .. 8 slots, shared
targets, steal chains of depth 1 .. 6 with their members in one block, in two, split at every link, and with the last one in block 2,
crowds after one to nine targets.  Both orders must end in the picks of the definition (sources in id order).  It prints the largest
number of extra sweeps the merged order needed.  Built with the address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_serial_and_merged_sweeps_reach_the_same_fix_point(tmp_path):
    exe = str(tmp_path / "spread_fixpoint_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "spread_fixpoint_probe.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    n, extra, ok = p.stdout.split()
    assert ok == "ok" and int(n) > 5000   # instances actually compared
    print("largest number of extra sweeps of the merged order:", int(extra))
