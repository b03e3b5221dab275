"""tests/lammax_ref.py on the CPU: the recurrences are the oracle's, every case of tests/test_gpu_lambda_max.py is a
sharp one on the reference alone, and the GPU tolerance has teeth. No GPU.

For every GPU case, in float64 and in long double: both CGs stop after exactly K = 4 iterations, with the residual
at iteration K - 1 at least 100 times the stop threshold and at iteration K at most 1 / 100 of it (1e-4 relative for
the released package's CG, 0.01 absolute for the research code's), and max|D x| of the iterate agrees with the closed
form to 1e-10 relative. Measured over the 120 cases: the residuals at K - 1 are 1.3e-2 .. 4.9e-2 relative and
16 .. 32 absolute, at K at most 1.1e-10 and 1.1e-12; the closed form is met to 6.5e-13 in float64 and 1e-14 in long
double. The GPU bound, 1e-9 relative (the project's theta tolerance), sits a factor 1e3 above that.

Coverage: for every block of every weighted (p, order), and for every effective set S' of every unweighted one, one
small case has the first row attaining max|D x| in that block (in a block with that S'; blocks of equal S' and
weight have equal rows, which no maximum tells apart), so a k_dmaxabs that drops or mis-weights any one block fails
the GPU test.

Teeth, each moving lambda_max by more than 1e-9 relative: the argmax block dropped from max|D x| (12 % .. 100 %); a
block weight off by 1e-9 relative in the operator (cS[S'] = sum w_b^2, which launch_apply_A's stencil weights come
from), on the steered cases where that block carries the eigenvalues (1.9e-9 .. 2.0e-9; the same error in
k_dmaxabs's own weight moves the value by 1e-9 exactly, at the tolerance and not beyond it); op 2's beta applied
to the wrong vector, p = p + beta r (both CGs run to 100 iterations or more and miss by 3.5e-4 at least)."""
import numpy as np
import pytest

import lammax_ref as L
from oracle import mvtv_oracle as O

LD = np.longdouble
RTOL_GPU = 1e-9   # tests/test_gpu_lambda_max.py
SPECS = L.specs()


@pytest.mark.parametrize("m,deltas,order,unit", [([9], None, "cpp", False), ([7, 5], [0.3, 0.7], "cpp", False),
                                                 ([6, 6, 6], [0.5, 0.25, 0.125], "cpp", False),
                                                 ([5, 5, 7], [0.2, 0.3, 0.4], "cpp", True),
                                                 ([4, 4, 4, 5], [0.5, 0.25, 0.125, 0.3], "cpp", False),
                                                 ([6, 5], None, "py", False),
                                                 ([5, 5, 5], [0.5, 0.25, 0.125], "py", False)])
def test_recurrences_are_the_oracles(m, deltas, order, unit):
    """on random data of zero mean (the research code's CG breaks down on an inconsistent system), over the oracle's
    own sparse A: bit for bit, many iterations"""
    weighted = (deltas is not None) and not unit
    D = O.build_D(m, O.block_table(len(m), deltas if weighted else None, order, unit_weights=unit))
    A = (D.T @ D).tocsr()
    b = np.random.default_rng(61).standard_normal(D.shape[1])
    b -= b.mean()
    x, it, hist = L.cg_rcpp(lambda v: A @ v, b)
    assert (5.0 * float(np.max(np.abs(D @ x))), it) == O.lam_max_pinv_rcpp(D, b) and len(hist) == it
    x, it, hist = L.cg_cpp(lambda v: A @ v, b)
    assert (float(np.max(np.abs(D @ x))), it) == O.lam_max_pinv_cpp(D, b) and len(hist) == it > L.K


@pytest.mark.parametrize("spec", [s for s in SPECS if s[5] is None and s[0] in L.SMALL], ids=L.spec_id)
def test_modes_are_eigenvectors_with_the_symbols_eigenvalues(spec):
    from oracle import spectral_ld as SLD
    c = L.case(spec)
    sym = SLD.dtd_symbol_ld(c.m, c.deltas, c.order, c.weighted)
    A = L.operator(c.m, c.blocks, LD)
    for k, lam in zip(c.ks, c.lam):
        assert abs(lam - sym[k]) <= 1e-17 * abs(sym[k])
        v = L.combine(c.m, [k], [1.0])
        assert float(np.max(np.abs(A(v) - lam * v))) <= 1e-16 * float(lam)


@pytest.mark.parametrize("spec", SPECS, ids=L.spec_id)
def test_every_gpu_case_is_sharp_on_the_reference(spec):
    c = L.case(spec)
    lm_r, lm_c, _ = c.closed_form
    assert min(float(v) for v in c.lam) > 0 and len({float(v) for v in c.lam}) == L.K
    # the K-component model agrees: the full problem behaves as exact arithmetic says
    assert c.model_rcpp[L.K - 2] >= 100 * L.RTOL_RCPP and 16.0 <= c.model_cpp[L.K - 2] < 32.0
    for dtype in (np.float64, LD):
        A = L.operator(c.m, c.blocks, dtype)
        x, it, hist = L.cg_rcpp(A, c.b, dtype)
        err = abs(5.0 * float(c.max_abs_D(x)[0]) - lm_r) / lm_r
        print(f"{c.name} {dtype.__name__} rcpp: {it} iterations, residual {hist[-2]:.2e} -> {hist[-1]:.2e}, "
              f"to the closed form {err:.1e}")
        assert it == L.K
        assert hist[L.K - 2] >= 100 * L.RTOL_RCPP and hist[L.K - 1] <= L.RTOL_RCPP / 100
        assert err <= 1e-10
        x, it, hist = L.cg_cpp(A, c.b, dtype)
        err = abs(float(c.max_abs_D(x)[0]) - lm_c) / lm_c
        print(f"{c.name} {dtype.__name__} cpp: {it} iterations, residual {hist[-2]:.2e} -> {hist[-1]:.2e}, "
              f"to the closed form {err:.1e}")
        assert it == L.K
        assert hist[L.K - 2] >= 100 * L.ATOL_CPP and hist[L.K - 1] <= L.ATOL_CPP / 100
        assert err <= 1e-10


def test_every_block_holds_the_argmax_in_some_case():
    hit_block, hit_sp = set(), set()
    for s in SPECS:
        m, order, weighted, _, _, target = s
        if target is None:
            continue
        c = L.case(s)
        blk = c.closed_form[2]
        if weighted:
            assert blk == target, L.spec_id(s)
            hit_block.add((len(m), order, blk))
        else:
            assert c.blocks[blk].Sp == target, L.spec_id(s)
            hit_sp.add((len(m), order, target))
    for p in (1, 2, 3, 4):
        for order in ("cpp", "py"):
            if not (p == 1 and order == "py"):
                nb = len(O.block_table(p, [1.0] * p, order))
                assert {t for q, o, t in hit_block if (q, o) == (p, order)} == set(range(nb))
            sps = {blk.Sp for blk in O.block_table(p, None, order, unit_weights=True)}
            assert {t for q, o, t in hit_sp if (q, o) == (p, order)} == sps


STEERED_W = [s for s in SPECS if s[5] is not None and s[2]]
SMALL_PLAIN = [s for s in SPECS if s[5] is None and s[0] in L.SMALL]


@pytest.mark.parametrize("spec", SMALL_PLAIN + STEERED_W, ids=L.spec_id)
def test_gpu_tolerance_has_teeth(spec):
    c = L.case(spec)
    lm_r, lm_c, blk = c.closed_form
    # (1) the argmax block missing from max|D x|
    if len(c.blocks) > 1:
        rest = [b for i, b in enumerate(c.blocks) if i != blk]
        dropped = float(c.max_abs_D(c.x_exact, rest)[0])
        assert abs(dropped - lm_c) / lm_c > RTOL_GPU
        print(f"{L.spec_id(spec)}: block {blk} dropped from max|D x|: {abs(dropped - lm_c) / lm_c:.1e}")
    # (2) its weight off by 1e-9 in the operator
    if spec in STEERED_W:
        bad = [O.Block(b.b, b.S, b.Sp, b.w * (1.0 + 1e-9) if i == blk else b.w) for i, b in enumerate(c.blocks)]
        lam = L.eigenvalues(c.m, bad, c.ks)
        x = L.combine(c.m, c.ks, [LD(a) / l for a, l in zip(c.coef, lam)])
        moved = abs(float(c.max_abs_D(x)[0]) - lm_c) / lm_c
        print(f"{L.spec_id(spec)}: weight of block {blk} + 1e-9 in the operator: {moved:.2e}")
        assert moved > RTOL_GPU
    # (3) p = p + beta r
    A = L.operator(c.m, c.blocks, np.float64)
    for cg, ref, scale in ((L.cg_rcpp, lm_r, 5.0), (L.cg_cpp, lm_c, 1.0)):
        x, it, _ = cg(A, c.b, beta_on_r=True)
        moved = abs(scale * float(c.max_abs_D(x)[0]) - ref) / ref
        print(f"{L.spec_id(spec)}: {cg.__name__} with p = p + beta r: {it} iterations, value off by {moved:.1e}")
        assert it != L.K or moved > RTOL_GPU
