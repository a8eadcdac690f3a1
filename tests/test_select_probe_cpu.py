"""The packed-prefix pool select (cygym_amd/csrc/cg_select.hpp: cg_prefix_pack / cg_prefix_word) on the host.

Block / unblock at a compile-time size finds the word of the chosen pool entry from the running popcounts the count left
behind instead of reading the row's words a second time.  The arithmetic is host-and-device code; tests/select_probe.cpp
runs it against the plain range_popc / range_select semantics for W = 9 and W = 3, every (a & 31, b & 31) a row of length
1, 31, 32, 33, 255 or 256 (and 2, 34, 47, 62-65, 95, 96, 128, 254: three full words at W = 3) can have within W words, all-zero, all-one and random words, both `want` values and every rank
in range -- built with the address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_prefix_select_matches_range_select(tmp_path):
    exe = str(tmp_path / "select_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cygym_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "select_probe.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    n, ok = p.stdout.split()
    assert ok == "ok" and int(n) > 100000   # counts and selects actually compared
