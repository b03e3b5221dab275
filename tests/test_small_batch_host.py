"""Host side of the batched small-mesh fits (mvtv_path_batch, multivartv_amd/csrc/mvtv_small.hip): no GPU.

1. The transcription (tests/small_batch_cases.py) of the admission formula, the workgroup-size rule and the LDS rule
   agrees with the constants in mvtv_internal.h; the GPU cases reach every instantiation an admitted mesh can reach,
   which are exactly the ones the launcher dispatches, and both sides of every bound.
2. Every GPU case that asserts iteration counts is decided, on the reference alone (mvtv_oracle.admm_rcpp, SuperLU,
   record=True), at least 1e-6 (relative) away from each threshold: r against 10 s, s against 10 r, r against eps_pri,
   s against eps_dual (the rule of DESIGN.md §2.2). A case that misses it is replaced, not loosened.
"""
import os
import re

import numpy as np
import pytest

import small_batch_cases as S
from oracle import mvtv_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multivartv_amd", "csrc")
MARGIN = 1e-6


def _const(name):
    src = open(os.path.join(CSRC, "mvtv_internal.h")).read()
    return int(re.search(rf"constexpr \w+ {name} = (\d+);", src).group(1))


def test_constants_are_the_librarys():
    assert _const("kSmallChunk") == S.CHUNK
    assert _const("kSmallMaxN") == S.MAX_N
    assert _const("kSmallMaxN4") == S.MAX_N4
    assert _const("kSmallZLds") == S.Z_LDS_WORDS
    src = open(os.path.join(CSRC, "mvtv_internal.h")).read()
    assert "return N <= 256 ? 64 : (N <= 1024 ? 256 : 1024);" in src
    assert [S.nt_rule(n) for n in (2, 256, 257, 1024, 1025, 4096)] == [64, 64, 256, 256, 1024, 1024]


def test_every_node_has_a_thread_and_the_lds_fits():
    """At most 4 nodes a thread (2 at p = 4, NT = 1024) and at most 160 KiB of LDS a workgroup, at every bound."""
    for p in (1, 2, 3, 4):
        cap = S.MAX_N4 if p == 4 else S.MAX_N
        for N in (2 ** p, 256, 257, 1024, 1025, cap):
            if N > cap:
                continue
            nt = S.nt_rule(N)
            assert N <= nt * (2 if (p == 4 and nt == 1024) else 4)
            for nb in {S.n_blocks(p, o, w) for o in ("cpp", "py") for w in (True, False)}:
                z = nb * N if nb * N <= S.Z_LDS_WORDS else 0
                assert 8 * (N + 2 * (nt // 64) * 3 + z) <= 160 * 1024


def test_gpu_cases_reach_every_instantiation():
    reached = {S.instantiation(m, o, w) for (m, o, w, _) in S.single_cases()}
    reached |= {S.instantiation(m) for m in S.PATH_SHAPES}
    assert reached == S.reachable_instantiations()
    src = open(os.path.join(CSRC, "mvtv_small.hip")).read()
    dispatched = set(re.findall(r"go\((k_admm_small<\d, \d+, (?:true|false)>)\)", src))
    assert dispatched == S.reachable_instantiations()


def test_gpu_cases_sit_on_both_sides_of_every_bound():
    assert S.admitted([4096]) and [4096] in S.SHAPES
    assert not S.admitted([4097]) and [4097] in S.REFUSED_SHAPES
    assert S.admitted([6] * 4) and [6] * 4 in S.SHAPES
    assert not S.admitted([7] * 4) and [7] * 4 in S.REFUSED_SHAPES
    Ns = {int(np.prod(m)) for m in S.SHAPES}
    assert {256, 1024} <= Ns and any(256 < n < 1024 for n in Ns) and any(1024 < n < 4096 for n in Ns)
    # the LDS rule at p = 3: 11^3 below, 16^3 above; at p = 4: 5^4 below, 4 x 4 x 4 x 16 above
    assert 7 * 11 ** 3 <= S.Z_LDS_WORDS < 7 * 16 ** 3
    assert 15 * 5 ** 4 <= S.Z_LDS_WORDS < 15 * 1024


@pytest.mark.parametrize("c", S.single_cases(), ids=S.case_id)
def test_single_fit_decisions_have_margin(c):
    res = S.slu_single(c)
    assert 2 <= res.iters < 3000
    assert S.margins(res.history) >= MARGIN, (res.iters, S.margins(res.history))


@pytest.mark.parametrize("m", S.PATH_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_path_decisions_have_margin(m):
    out = S.slu_path(m)
    assert all(2 <= r.iters < 3000 for r in out)
    assert min(S.margins(r.history) for r in out) >= MARGIN
    assert all(len(r.history) == r.iters for r in out) and O.admm_rcpp.__name__ == "admm_rcpp"


def test_mixed_ending_cases_have_margin():
    """The members of the mixed-endings batch and their max_counter = 5 runs: one stops within 5 iterations, the
    others after very different counts, each decided with margin."""
    iters = []
    for j in range(len(S.mixed_members())):
        full, capped = S.slu_member(j), S.slu_member(j, 5)
        assert S.margins(full.history) >= MARGIN and S.margins(capped.history) >= MARGIN
        assert capped.iters == min(full.iters, 5)
        iters.append(full.iters)
    assert min(iters) < 5 and sorted(iters)[1] > 5 and max(iters) > 4 * sorted(iters)[1], iters
