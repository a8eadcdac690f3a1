"""The arrival-period test of every tick (cygym_amd/csrc/cg_period.hpp) on the host.

At the compile-time sizes the tick kernels form floor(sqrt(n_active) / 2) by counting thresholds and test `step_num % period == 0`
with a float quotient and one multiply instead of a division sequence.  Both are host-and-device code; tests/period_probe.cpp runs
them against plain loops: every n up to 64 / 128 / 192 / 256, and every step_num below 2^20 against the periods 1 .. 300, the
powers of two from 2^9 to 2^30 with their neighbours and 2^31 - 1, each with the reciprocal two units in the last place low,
correctly rounded and two high (the device instruction is good to one) -- built with the address and undefined-behaviour
sanitizers, as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_period_helpers_match_plain_loops(tmp_path):
    exe = str(tmp_path / "period_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cygym_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "period_probe.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    n, ok = p.stdout.split()
    assert ok == "ok" and int(n) > 1000000000   # every (step_num, period, reciprocal) actually compared
