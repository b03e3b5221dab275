"""cv.mbs_impl(batched=True, batch_cosine=2): the final path and the CV folds as one Problem.path_batch call with the
cosine-preconditioned PCG (k_admm_cos<..., true>; the scattered members have W != I), against
mvtv_oracle.mbs_impl_rcpp with the fold labels of cv.kfoldinds, on the shapes of tests/test_gpu_small_batch_cv.py
(1-D m = 20, n = 100; 10 x 10, n = 100; 4^3, n = 300), folds 1 and 5, 5 lambdas, at that file's 1e-7. The launch log
shows only the new kernel for the paths (the folds = 1 refit goes through Problem.admm as before)."""
import ctypes

import numpy as np
import pytest

import small_batch_cases as S
import small_cos_model as M
from oracle import mvtv_oracle as O

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import _lib, cv  # noqa: E402

pytestmark = pytest.mark.gpu

LAMS = S.LAMS


def _scattered(n, p, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(n, p))
    f = np.where(np.all(x > 0.6, axis=1), 1.0, 0.0)
    return x, f + 0.3 * rng.standard_normal(n)


def _log_now():
    """The launch log so far, parsed as _lib.launch_log does, without ending the recording."""
    L = _lib.lib()
    n = int(L.mvtv_launch_log_read(None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    L.mvtv_launch_log_read(buf, n + 1)
    out = []
    for line in buf.value.decode().splitlines():
        assert not line.startswith("#"), line   # the ring has not overflowed
        name, grid, block = line.split("\t")
        out.append((name, tuple(int(v) for v in grid.split()), tuple(int(v) for v in block.split())))
    return out


@pytest.mark.parametrize("folds", [1, 5])
@pytest.mark.parametrize("m,n", [([20], 100), ([10, 10], 100), ([4, 4, 4], 300)], ids=["20", "10x10", "4x4x4"])
def test_batched_cosine_mbs_impl_matches_oracle(m, n, folds, monkeypatch):
    x, y = _scattered(n, len(m), seed=10 * len(m) + folds)
    # the log is read when the folds = 1 refit begins (it can overrun the log's ring)
    at_refit = []
    plain_admm = mv.Problem.admm

    def admm(self, *a, **kw):
        at_refit.append(_log_now())
        return plain_admm(self, *a, **kw)
    monkeypatch.setattr(mv.Problem, "admm", admm)
    with _lib.launch_log() as log:
        out = cv.mbs_impl(x, y, m, lambdas=LAMS, folds=folds, seed=11, group=False, batched=True, batch_cosine=2)
    fi = cv.kfoldinds(len(y), folds, 11) if folds > 1 else None
    ref = O.mbs_impl_rcpp(x, y, m, LAMS, foldinds=fi, folds=folds)
    assert out["lambda_minmse_ind"] == ref["best"] + 1
    assert np.allclose(out["cv.mses"], ref["cv_mses"], rtol=1e-7, atol=0)
    scale = np.max(np.abs(ref["best_theta"]))
    assert np.max(np.abs(out["theta_hat"] - ref["best_theta"])) <= 1e-7 * scale
    for i, r in enumerate(ref["final"]):
        assert np.max(np.abs(out["models"][i]["theta_hat"] - r.theta)) <= 1e-7 * max(1.0, np.max(np.abs(r.theta)))
    assert len(at_refit) == (1 if folds == 1 else 0)
    log = at_refit[0] if folds == 1 else log
    name = M.loop_name(m, True)
    nbatch = 1 + (folds if folds > 1 else 0)
    paths = [e for e in log if e[0].startswith("k_admm_cos")]
    assert paths and all(e == (name, (nbatch, 1, 1), (64, 1, 1)) for e in paths)
    first, last = log.index(paths[0]), len(log) - 1 - log[::-1].index(paths[-1])
    assert log[first:last + 1] == paths
    loop = ("k_admm_small", "k_edge_update", "k_edge3d", "k_gather", "k_pcg", "k_admm_control", "k_admm3d", "k_cg3d")
    assert not [e for e in log if e[0].startswith(loop)]


def test_default_is_unchanged():
    """batch_cosine defaults to 0: the paths run in k_admm_small."""
    x, y = _scattered(100, 2, seed=4)
    with _lib.launch_log() as log:
        cv.mbs_impl(x, y, [10, 10], lambdas=LAMS[:2], folds=2, seed=11, group=False, batched=True)
    assert [e for e in log if e[0].startswith("k_admm_small")] and not [e for e in log if e[0].startswith("k_admm_cos")]
