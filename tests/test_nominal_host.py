"""tests/nominal_ref.py on the CPU: the nominal D is the operator the nominal block orders promise, and the ADMM
parity cases of tests/test_gpu_nominal.py can ask for exact iteration counts.

* D^T D of the helper's D equals sum_S w_S^2 (x)_{j in S} L_j (1-D Neumann Laplacians) on meshes of unequal extents,
  and its eigenvalues on the cosine products are the helper's symbol.
* For p <= 2 both rules give the same sets: the helper's D is ``build_D``'s.
* On 5 x 5 x 5, which the reference accepts, it differs from the reference's D in exactly the blocks whose nominal
  set misses dim 0 (min S > 0) and has more than one dim.
* Every variant-B parity case's SuperLU run keeps each adapt and stopping comparison at least 1e-6 relative from its
  threshold, and so do the variant A and C cases.
"""
import numpy as np
import pytest

import nominal_ref as R
from oracle import mvtv_oracle as O

MESHES = [(6, 5, 4), (70, 9, 5), (5, 4, 3, 2), (12, 10, 7)]


@pytest.mark.parametrize("order,weighted", R.LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("m", MESHES, ids=lambda m: "x".join(map(str, m)))
def test_dtd_is_the_kronecker_sum(m, order, weighted):
    blks = R.blocks_of(m, order, weighted)
    D = R.build_D(list(m), blks)
    E, rows = R.info(m, blks)
    assert D.shape == (E, int(np.prod(m)))
    assert len({s for _, s, _ in rows}) == len(rows)   # no two blocks share a set
    dtd, kron = (D.T @ D).tocsr(), R.kron_dtd(m, blks)
    scale = abs(kron).max()
    assert abs(dtd - kron).max() <= 1e-14 * scale
    # the symbol: D^T D v_k = sym[k] v_k on a cosine product v_k
    sym = R.dtd_symbol(m, blks, np.float64)
    k = tuple(int(v) - 1 - (j % 2) for j, v in enumerate(m))
    v = np.ones([1] * len(m))
    for j, mj in enumerate(m):
        shape = [1] * len(m)
        shape[j] = mj
        v = v * np.cos(np.pi * k[j] * (np.arange(mj) + 0.5) / mj).reshape(shape)
    v = v.ravel(order="F")
    assert np.max(np.abs(dtd @ v - sym[k] * v)) <= 1e-13 * abs(sym[k]) * np.max(np.abs(v))


# (Python's create_D with deltas has no block at p = 1)
@pytest.mark.parametrize("m,order,weighted", [(m, o, w) for m in [(20,), (33, 31)] for o, w in R.LAYOUTS
                                              if not (len(m) == 1 and o == "py" and w)], ids=lambda v: str(v))
def test_same_D_up_to_two_dims(m, order, weighted):
    ref = O.build_D(list(m), O.block_table(len(m), R.deltas_of(m) if weighted else None, order,
                                           unit_weights=not weighted))
    D = R.build_D(list(m), R.blocks_of(m, order, weighted))
    assert D.shape == ref.shape and abs(D - ref).max() == 0.0


def test_differs_from_the_reference_where_min_S_is_positive():
    m = [5, 5, 5]
    tab = O.block_table(3, R.deltas_of(m), "cpp")
    O.check_dims(m, tab)
    differ = []
    for ref, nom in zip(tab, R.blocks_of(m)):
        assert (ref.b, ref.w, ref.S) == (nom.b, nom.w, nom.S) and nom.Sp == nom.S
        a, b = O.build_block(m, ref), O.build_block(m, nom)
        differ.append(a.shape != b.shape or abs(a - b).max() != 0.0)
    assert differ == [len(b.S) >= 2 and b.S[0] > 0 for b in tab]
    assert [b.S for b, d in zip(tab, differ) if d] == [(1, 2)]


@pytest.mark.parametrize("c", R.admm_cases(), ids=R.case_id)
def test_parity_cases_have_margins(c):
    res, margin = R.slu(c)
    print(R.case_id(c), res.iters, res.rho, f"{margin:.2e}")
    assert res.iters >= 2 and margin >= R.MARGIN


@pytest.mark.parametrize("v", R.VARIANT_CASES, ids=lambda v: f"{v[0]}-{'x'.join(map(str, v[1]))}")
def test_variant_cases_have_margins(v):
    res, margin = R.variant_run(v)
    print(v, res.iters, res.rho, f"{margin:.2e}")
    assert res.iters >= 2 and margin >= R.MARGIN
