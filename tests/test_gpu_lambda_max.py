"""Problem.lambda_max / lambda_max_cpp (mvtv_lambda_max / mvtv_lambda_max_cpp: k_cg_vec ops 0 to 3, the W_NONE
stencil, k_dmaxabs<P, ORD>) where the reference's CG is well conditioned, so that the check can be sharp: O^T y is a
sum of K = 4 high-frequency eigenvectors of D^T D, both CGs stop after exactly K iterations and lambda_max is a closed
form (tests/lammax_ref.py; on the reference alone, with margins and teeth: tests/test_lammax_ref_host.py).

Asserted per case: the iteration count is K, and the value is within 1e-9 relative (the project's theta tolerance) of
the closed form; the reference's own float64 run sits below 1e-12 (achieved on the GPU: 1.8e-13 and 3.4e-15).
Cases: 600, 1 048 876 (the streaming grid wraps), 40 x 33, 1030 x 520, 12 x 12 x 9, 65 x 65 x 130, 6 x 6 x 6 x 5 and
28 x 28 x 28 x 25 in the four block orders, and on the small meshes one case per block (weighted orders) or per
effective set S' (unweighted) whose max|D x| lies in that block, steered by the deltas or by the dims the modes vary
along. The errors go to $MVTV_PARITY_LOG.

The 5e-3 and 1e-2 checks on scattered data (tests/test_gpu_cv.py, tests/test_gpu_cxx_cpp.py) stay as they are."""
import numpy as np
import pytest

import lammax_ref as L
from conftest import log_parity

mv = pytest.importorskip("multivartv_amd")

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.mark.parametrize("spec", L.specs(), ids=L.spec_id)
def test_lambda_max_is_the_closed_form(spec):
    m, order, weighted, deltas, _, _ = spec
    c = L.case(spec)
    lm_r, lm_c, blk = c.closed_form
    with mv.Problem(list(m), c.b, deltas=list(deltas), order=mv.ORDER_CPP if order == "cpp" else mv.ORDER_PY,
                    weighted=weighted) as P:
        assert P.nb == len(c.blocks)
        v_r, it_r = P.lambda_max()
        v_c, it_c = P.lambda_max_cpp()
    e_r, e_c = abs(v_r - lm_r) / lm_r, abs(v_c - lm_c) / lm_c
    print(f"{L.spec_id(spec)}: lambda_max {it_r} iterations, off the closed form by {e_r:.2e}; lambda_max_cpp {it_c}, "
          f"{e_c:.2e}; argmax in block {blk}")
    log_parity(f"lambda_max/{L.spec_id(spec)}", rcpp=e_r, cpp=e_c, it_rcpp=it_r, it_cpp=it_c, block=blk)
    assert it_r == L.K and it_c == L.K
    assert e_r <= RTOL
    assert e_c <= RTOL
    assert np.isfinite(v_r) and np.isfinite(v_c)
