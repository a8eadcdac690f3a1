"""What stands in front of the first scalar wait of the per-tick kernels' prologue, read from the gfx950 assembly of a cross-compile
(no GPU needed; the kernels and the slicing are those of test_prologue_isa_cpu.py).

The first `s_waitcnt lgkmcnt(0)` of a wave is on every env's chain, and scalar loads return out of order: that wait lasts as long
as the slowest request in front of it.  It must therefore cover the hot block alone -- the eight loads of hot_batch (cg_tick.hpp;
nine in the full-feature kernels) -- and the one-dword requests for the argument lines of later phases (karg_prefetch) follow
behind it, still in the entry block (before the first exec-mask region or branch), so that they are outstanding while the gather
and DMA addresses issue and are back at the wait the staging barrier has anyway.  Before this layout all 18 loads stood in front
of the first wait, and the prologue had two full waits before the barrier (the first one, and the one in front of s_barrier).

The line requests all target one scratch SGPR whose value nobody reads.  The compiler keeps that register allocated up to the
statement behind the barrier that waits for the requests; were it spilled or re-used in between, a load would land in a register
that holds something else by then.  So the register may appear in no other instruction of the prologue."""
import re

import pytest

from test_prologue_isa_cpu import PARENT, _targs, prologues   # noqa: F401  (the module-scoped fixture that compiles the kernels)

FULL_WAIT = re.compile(r"s_waitcnt\b.*lgkmcnt\(0\)")
WAITS_BEFORE = 2   # full waits in front of the barrier before the line requests moved (all three kernels)


def _first(ins, pred):
    return next((i for i, s in enumerate(ins) if pred(s)), len(ins))


@pytest.mark.parametrize("key", list(PARENT), ids=lambda k: "step_kernel<" + _targs(k) + ">")
def test_first_wait_covers_the_hot_block_alone(prologues, key):   # noqa: F811
    ins = prologues[key]
    wait0 = _first(ins, lambda s: FULL_WAIT.match(s) is not None)
    region = _first(ins, lambda s: s.startswith("s_and_saveexec") or s.startswith("s_cbranch"))
    loads = [i for i, s in enumerate(ins) if s.startswith("s_load")]
    front = [i for i in loads if i < wait0]
    behind = [i for i in loads if i > wait0]
    waits = sum(FULL_WAIT.match(s) is not None for s in ins)
    print(key, {"first_wait": wait0, "s_load_in_front": len(front), "s_load_behind": len(behind), "last_s_load": loads[-1],
                "first_region": region, "full_waits": waits})
    assert wait0 < len(ins), "no full scalar wait in the prologue"
    assert 0 < len(front) <= 9, (len(front), wait0)
    assert behind and all(i < region for i in behind), (behind, region)   # the line requests: behind the wait, in the entry block
    assert waits <= WAITS_BEFORE, waits


@pytest.mark.parametrize("key", list(PARENT), ids=lambda k: "step_kernel<" + _targs(k) + ">")
def test_line_requests_share_one_register_that_nothing_else_touches(prologues, key):   # noqa: F811
    ins = prologues[key]
    wait0 = _first(ins, lambda s: FULL_WAIT.match(s) is not None)
    req = [(i, re.match(r"s_load_dword s(\d+), ", s)) for i, s in enumerate(ins) if i > wait0 and s.startswith("s_load")]
    assert req and all(m is not None for _, m in req), [ins[i] for i, _ in req]   # one dword each
    regs = {int(m.group(1)) for _, m in req}
    assert len(regs) == 1, regs
    r = regs.pop()

    def touches(s):
        if re.search(rf"\bs{r}\b", s):
            return True
        return any(int(a) <= r <= int(b) for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", s))
    others = [f"{i}: {s}" for i, s in enumerate(ins) if i > wait0 and touches(s) and i not in {j for j, _ in req}]
    assert not others, (f"s{r}", others)
