"""The K loop of the ping-pong GEMM (gemm3_kernel) across the boundary between its bulk loop (steps 0 .. nk-3: whole K-tiles of the current
output tile only) and its last two general steps (ragged last K-tile, prefetch of the next output tile).

Every case is exact: integer operands (the Tier 1 generators of test_gemm_ops.py) keep every fp32 partial sum below 2^24, so the result must
equal the float64 product — rounded once to bf16 where the output is bf16, the comparison test_gemm_ops._tier1_case makes — whatever the
split of the K steps between the two loops.  The static and the dynamic tile schedule are both held to that one reference, which makes them
agree bit for bit; the grouped cases compare the two schedules' output buffers directly as well.

The cases run in child processes with UCFVIT_GEMM_STAGGER = 0 (the staggered kernel takes nothing) and UCFVIT_GEMM_CUS = 8 (eight
workgroups: with nine or more tiles some workgroup takes a second tile, so the prefetch of a next tile follows a K loop of every length),
the pattern of test_gemm_cus_values_bit_identical.

What the host route allows (csrc/gemm_route.h) shapes the table:
  * a single GEMM goes to gemm3_kernel from 192 output tiles of 256 x 256 on, so the single-GEMM cases are 16200 x 520 (64 x 3 tiles, clamped
    edge rows and columns) and, where the column sums must stay below 2^24, 700 x 16392 (3 x 65 tiles); each case first asks
    ucfvit_gemm_route and asserts a "g3-" answer.  768 x 768 and 696 x 520 reach the kernel through ucfvit_gemm_grouped, which has no tile
    minimum (and no route query: the cases keep to the conditions ucfvit_gemm_grouped states for its one-launch path);
  * K < 128 never reaches a DMA kernel, so nk = 1 (K = 64, 61) and K = 125 cannot run on gemm3_kernel at all: asserted from the
    route below.  nk = 2 (no bulk step), 3 (one), 4 and 5 (several) are K = 128, 192, 256, 320;
  * a ragged K must be a multiple of 8 when an operand is K-contiguous: 136 and 200 there, 189, 253 and 317 for KS x KS;
  * a 256 x 256 plan is never split along K: no split-K case.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (os.path.join(ROOT, "ucf-vit_amd"), ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from test_gemm_ops import (F32, KC, KS, MUL_AUX, Case, _bits, _child, _desc, _group_check, _group_items, _lib_route, _ops,  # noqa: E402
                           _tier1_case)

gpu = pytest.mark.gpu
K_WHOLE = (128, 192, 256, 320)            # nk = 2, 3, 4, 5: zero, one, two and three bulk steps
K_RAGGED8 = (136, 200)                    # nk = 3, 4 with a last K-tile of 8
K_RAGGED = (189, 253, 317)                # nk = 3, 4, 5 with a last K-tile of 61 (KS x KS only)
M1, N1 = 16200, 520                       # 64 x 3 tiles, 72 valid rows in the last tile row, 8 valid columns in the last tile column
M2, N2 = 700, 16392                       # 3 x 65 tiles; 700 rows keep the column sums exact


def _single_cases(group):
    out = []
    if group == "kckc":
        for K in K_WHOLE + K_RAGGED8:
            out += [Case("g3-PLAIN", M1, N1, K), Case("g3-RESIDUAL", M1, N1, K, bias=True, res=True), Case("g3-MUL_AUX", M1, N1, K, act=MUL_AUX)]
    elif group == "kckc_cs":
        for K in K_WHOLE + K_RAGGED8:
            out += [Case("g3-PLAIN+CS", M2, N2, K, cs="ow"), Case("g3-MUL_AUX+CS", M2, N2, K, act=MUL_AUX, cs="ow")]
    elif group == "mixed":
        for K in K_WHOLE + K_RAGGED8:
            out += [Case("g3-GENERIC", M1, N1, K, la=KC, lb=KS), Case("g3-GENERIC", M1, N1, K, la=KS, lb=KC, out32=True)]
    elif group == "ksks":
        for K in K_WHOLE + K_RAGGED:
            out.append(Case("g3-GENERIC", M1, N1, K, la=KS, lb=KS, out32=True))
    return out


# (696, not 700: a KS operand's rows are its contiguous index and move in 16-byte pieces, so M % 8 == 0; 696 = 2 * 256 + 184)
GROUPED_SIZES = {2: [(768, 768), (696, 520)], 5: [(768, 768), (696, 520), (256, 256), (392, 264), (136, 128)]}


def _grouped(dyn):
    """KS x KS, fp32 out through ucfvit_gemm_grouped; returns the output buffers' bits"""
    ops = _ops()
    bits = []
    for K in K_WHOLE + K_RAGGED:
        for n, sizes in GROUPED_SIZES.items():
            for accs in (None, [i % 2 == 1 for i in range(n)]):
                assert K >= 128 and all(a >= 128 and b >= 128 and a % 8 == 0 and b % 8 == 0 for a, b in sizes)      # the one-launch path's conditions
                items = _group_items(sizes, K, 31 + K + n, F32, "int", accs)
                ops.wgrad_grouped([(dy, x, out, acc) for dy, x, out, acc, _, _ in items])
                _group_check(items, K, True, "kloop grouped")
                bits += [_bits(it[4]).cpu() for it in items]
    return bits


def _payload(group):
    ops = _ops()
    assert os.environ.get("UCFVIT_GEMM_CUS") == "8" and os.environ.get("UCFVIT_GEMM_STAGGER") == "0"
    per_sched = []
    for dyn in (False, True):
        assert ops.set_dynamic_tile_schedule(dyn) is dyn
        try:
            if group == "grouped":
                per_sched.append(_grouped(dyn))
                continue
            for c in _single_cases(group):
                name = _lib_route(c, _desc(c), dyn)
                assert name == c.branch and name.startswith("g3-"), f"{c.id}: routed to {name}, not to the ping-pong kernel"
                _tier1_case(c)
        finally:
            ops.set_dynamic_tile_schedule(False)
    if group == "grouped":
        assert len(per_sched[0]) == len(per_sched[1]) > 0
        for a, b in zip(*per_sched):
            assert torch.equal(a, b), "grouped: the static and the dynamic schedule differ"
    torch.cuda.synchronize()
    print("kloop", group, "ok")


@gpu
@pytest.mark.parametrize("group", ["kckc", "kckc_cs", "mixed", "ksks", "grouped"])
def test_gemm3_kloop_exact(group):
    r = _child([os.path.abspath(__file__), group], {"UCFVIT_GEMM_CUS": "8", "UCFVIT_GEMM_STAGGER": "0"}, 300)
    assert f"kloop {group} ok" in r.stdout


def test_gemm3_kloop_one_k_tile_is_not_routed_here():
    """K < 128 (nk = 1) goes to the first-generation kernels whatever the layouts and the size: the ping-pong K loop starts at nk = 2"""
    for la, lb in ((KC, KC), (KS, KS), (KC, KS), (KS, KC)):
        for K in (64, 120) + ((61, 125) if (la, lb) == (KS, KS) else ()):
            c = Case("", M1, N1, K, la=la, lb=lb, out32=True)
            for dyn in (False, True):
                assert _lib_route(c, _desc(c), dyn).startswith("v1-")
    for group in ("kckc", "kckc_cs", "mixed", "ksks"):          # the table of the GPU test, from the host alone
        for c in _single_cases(group):
            for dyn in (False, True):
                assert _lib_route(c, _desc(c), dyn) == c.branch, c.id


if __name__ == "__main__":
    if len(sys.argv) == 2:
        _payload(sys.argv[1])
    else:
        sys.exit("usage: test_gemm3_kloop.py kckc | kckc_cs | mixed | ksks | grouped")
