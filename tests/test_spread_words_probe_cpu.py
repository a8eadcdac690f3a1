"""The packed-word passes of the compile-time spread (cygym_amd/csrc/cg_spread_words.hpp) on the host.

At 256 devices attacker_spread_ct compacts its sources, forms its T words and candidate masks and applies the compromise flags on
one dword per lane -- four devices -- instead of one byte per lane and chunk.  Every bit expression of those passes is
host-and-device code; tests/spread_words_probe.cpp runs it against the byte-wise text that the other kernels keep: every (flag
byte, vulnerability byte) pair with every exploit bit in every byte position, the apply word at and around the two "no take"
values of a T word, and whole envs modelled lane by lane (source list, T table, the 32 bytes of candidate masks, the two lowest
candidates) with 0, 1, 2 and many candidates -- the lowest ones in the first byte and in the last, in one nibble, in neighbouring
lanes and across a chunk edge -- and source counts 0 .. 256.  Built with the address and undefined-behaviour sanitizers, as a
stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_helpers_match_the_byte_wise_text(tmp_path):
    exe = str(tmp_path / "spread_words_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cygym_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "spread_words_probe.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    n, ok = p.stdout.split()
    assert ok == "ok" and int(n) > 25000000   # every byte pair, exploit bit and position actually compared
