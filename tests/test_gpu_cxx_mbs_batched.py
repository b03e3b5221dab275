"""`mvtv_mbs --batched`: the C++ host API's mbs_impl with mbs_impl_options::batched (include/mvtv/solvers.hpp), the
whole CV as one mvtv_cv_batch call, against cv.mbs_impl(batched=True, device_cv=True) on a given grid. Both drive the
same C call; they differ in the members' constant starts (means summed sequentially in C++, pairwise in numpy) and the
PCG then stops at a discrete iteration, so the results agree to the 1e-7 of tests/test_gpu_cv.py, not to rounding
(test_batched_agrees_with_unbatched in tests/test_gpu_small_batch_cv.py gives the same reason). The index is compared
exactly, after the Python result's two smallest CV values are seen to lie >= 1e-5 apart.

Runs multivartv_amd/lib/mvtv_mbs (built by `make -C multivartv_amd/csrc`) as a child process."""
import os
import subprocess

import numpy as np
import pytest

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import cv  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(mv.__file__), "lib", "mvtv_mbs")
LAMBDAS = np.exp(np.linspace(np.log(2.0), np.log(0.02), 5))


def _run_cli(tmp_path, flag, x, y, m, folds, lambdas, seed=0):
    n, p = x.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    hdr = np.array([n, p, len(lambdas), folds, seed, 1, 0], dtype=np.int64)
    fin.write_bytes(b"".join([hdr.tobytes(), np.asarray(m, dtype=np.float64).tobytes(),
                              np.asfortranarray(x).tobytes(order="F"), y.astype(np.float64).tobytes(),
                              np.asarray(lambdas, dtype=np.float64).tobytes()]))
    r = subprocess.run([CLI, flag, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    b = fout.read_bytes()
    nl, ind, N, nn = np.frombuffer(b[:32], dtype=np.int64)
    v = np.frombuffer(b[32:], dtype=np.float64)
    out, o = {}, 0
    for name, k in (("lambdas", nl), ("cv", nl), ("model_mses", nl), ("theta", N), ("fitted", nn), ("resid", nn)):
        out[name] = v[o:o + k]
        o += k
    out["ind"] = int(ind)
    return out


def _problem(n, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(n, p))
    f = np.where(np.all(x > 0.55, axis=1), 1.0, 0.0)
    return x, f + 0.3 * rng.standard_normal(n)


def _gap(v):
    v = np.sort(np.asarray(v))
    return (v[1] - v[0]) / v[0]


@pytest.mark.parametrize("m,n,folds", [([12, 10], 500, 1), ([12, 10], 500, 3), ([4, 4, 4], 300, 5)],
                         ids=["12x10-f1", "12x10-f3", "4x4x4-f5"])
def test_cxx_batched_matches_python_device_cv(tmp_path, m, n, folds):
    x, y = _problem(n, len(m), seed=folds)
    ref = cv.mbs_impl(x, y, m, lambdas=LAMBDAS, folds=folds, seed=5, group=False, batched=True, device_cv=True)
    assert _gap(ref["cv.mses"]) >= 1e-5
    got = _run_cli(tmp_path, "--batched", x, y, m, folds, LAMBDAS, seed=5)
    np.testing.assert_array_equal(got["lambdas"], LAMBDAS)
    assert got["ind"] == ref["lambda_minmse_ind"]
    np.testing.assert_allclose(got["cv"], ref["cv.mses"], rtol=1e-7)
    scale = np.max(np.abs(ref["theta_hat"]))
    assert np.max(np.abs(got["theta"] - ref["theta_hat"])) <= 1e-7 * scale
    assert np.max(np.abs(got["fitted"] - ref["fitted"])) <= 1e-7 * scale
    assert np.max(np.abs(got["resid"] - ref["residuals"])) <= 1e-7 * scale
    np.testing.assert_allclose(got["model_mses"], [md["mse"] for md in ref["models"]], rtol=1e-7)


def test_cxx_batched_cosine_on_identity_data(tmp_path):
    """One point a node (W = I): under --batched=1 every member of the folds = 1 CV takes the exact cosine solve; the
    selection is that of --batched."""
    m = [12, 10]
    rng = np.random.default_rng(4)
    axes = [(np.arange(v) + 0.5) / v for v in m]
    g = np.meshgrid(*axes, indexing="ij")
    x = np.stack([a.reshape(-1, order="F") for a in g], axis=1)
    y = np.where(np.all(x > 0.55, axis=1), 1.0, 0.0) + 0.3 * rng.standard_normal(x.shape[0])
    a = _run_cli(tmp_path, "--batched", x, y, m, 1, LAMBDAS)
    b = _run_cli(tmp_path, "--batched=1", x, y, m, 1, LAMBDAS)
    assert _gap(a["cv"]) >= 1e-5
    assert a["ind"] == b["ind"]


def test_cxx_batched_refuses_a_large_mesh(tmp_path):
    x, y = _problem(400, 2, seed=1)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    hdr = np.array([400, 2, len(LAMBDAS), 1, 0, 1, 0], dtype=np.int64)
    fin.write_bytes(b"".join([hdr.tobytes(), np.array([100.0, 100.0]).tobytes(), np.asfortranarray(x).tobytes(order="F"),
                              y.tobytes(), LAMBDAS.tobytes()]))
    r = subprocess.run([CLI, "--batched", str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "batched" in r.stderr
