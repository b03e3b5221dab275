"""The C++ host API under the nominal difference sets: mvtv::mbs_impl with mbs_impl_options::nominal
(include/mvtv/solvers.hpp; the switch travels in mbs_cache into create_cache_objects' problem) and `mvtv_mbs --nominal`
on 300 scattered points over a 4 x 5 x 6 mesh, which the reference rule refuses, against the Python driver
(multivartv_amd.cv.mbs_impl(nominal=True)). Both drive the same C ABI, so on a given lambda grid they agree to rounding,
with the tolerances of tests/test_gpu_cxx_mbs.py: the chosen index exactly, theta / fitted / MSEs to 1e-12 (the
batched mode: the 1e-7 of tests/test_gpu_cxx_mbs_batched.py, for its reason).

Compiles tests/cpp/nominal_mbs_main.cpp against the built library, as tests/test_gpu_shims.py does for its driver."""
import os
import subprocess

import numpy as np
import pytest

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import cv  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multivartv_amd", "lib")
CLI = os.path.join(LIB, "mvtv_mbs")
M, N_PTS, FOLDS, SEED = [4, 5, 6], 300, 5, 3
LAMBDAS = np.exp(np.linspace(np.log(2.0), np.log(0.02), 5))


def _data():
    rng = np.random.default_rng(17)
    x = rng.uniform(0, 1, size=(N_PTS, 3))
    return x, np.where(np.all(x > 0.45, axis=1), 1.0, 0.0) + 0.5 * x[:, 0] + 0.3 * rng.standard_normal(N_PTS)


def _write_input(path, x, y):
    hdr = np.array([N_PTS, 3, len(LAMBDAS), FOLDS, SEED, 1, 0], dtype=np.int64)
    path.write_bytes(b"".join([hdr.tobytes(), np.asarray(M, dtype=np.float64).tobytes(),
                               np.asfortranarray(x).tobytes(order="F"), y.tobytes(), LAMBDAS.tobytes()]))


def _read_output(path):
    b = path.read_bytes()
    nl, ind, N, nn = np.frombuffer(b[:32], dtype=np.int64)
    v = np.frombuffer(b[32:], dtype=np.float64)
    out, o = {"ind": int(ind)}, 0
    for name, k in (("lambdas", nl), ("cv", nl), ("model_mses", nl), ("theta", N), ("fitted", nn), ("resid", nn)):
        out[name] = v[o:o + k]
        o += k
    return out


def _check(got, ref, batched=False):
    np.testing.assert_array_equal(got["lambdas"], LAMBDAS)
    assert got["ind"] == ref["lambda_minmse_ind"]
    if not batched:   # tests/test_gpu_cxx_mbs.py
        np.testing.assert_allclose(got["cv"], ref["cv.mses"], rtol=1e-12)
        np.testing.assert_allclose(got["theta"], ref["theta_hat"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["fitted"], ref["fitted"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["resid"], ref["residuals"], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["model_mses"], [md["mse"] for md in ref["models"]], rtol=1e-12)
        return
    # tests/test_gpu_cxx_mbs_batched.py: the members' constant starts are summed sequentially in C++ and pairwise in
    # numpy, and the in-workgroup PCG then stops at a discrete iteration
    v = np.sort(ref["cv.mses"])
    assert (v[1] - v[0]) / v[0] >= 1e-5
    np.testing.assert_allclose(got["cv"], ref["cv.mses"], rtol=1e-7)
    scale = np.max(np.abs(ref["theta_hat"]))
    assert np.max(np.abs(got["theta"] - ref["theta_hat"])) <= 1e-7 * scale
    assert np.max(np.abs(got["fitted"] - ref["fitted"])) <= 1e-7 * scale
    assert np.max(np.abs(got["resid"] - ref["residuals"])) <= 1e-7 * scale
    np.testing.assert_allclose(got["model_mses"], [md["mse"] for md in ref["models"]], rtol=1e-7)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nominal") / "nominal_mbs"
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "nominal_mbs_main.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", LIB, "-lmvtv", f"-Wl,-rpath,{LIB}", "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("batched", [False, True], ids=["plain", "batched"])
def test_cxx_mbs_impl_nominal(tmp_path, driver, batched):
    x, y = _data()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _write_input(fin, x, y)
    r = subprocess.run([driver, str(fin), str(fout)] + (["batched"] if batched else []), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["refused", "3"]   # the default options: MVTV_DIM_MISMATCH
    ref = cv.mbs_impl(x, y, M, lambdas=LAMBDAS, folds=FOLDS, seed=SEED, group=False, nominal=True, batched=batched,
                      device_cv=batched)
    _check(_read_output(fout), ref, batched)


def test_cli_nominal(tmp_path):
    x, y = _data()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _write_input(fin, x, y)
    r = subprocess.run([CLI, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "m[0] != m[1]" in r.stderr   # the default keeps the reference's refusal
    r = subprocess.run([CLI, "--nominal", str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ref = cv.mbs_impl(x, y, M, lambdas=LAMBDAS, folds=FOLDS, seed=SEED, group=False, nominal=True)
    _check(_read_output(fout), ref)
    r = subprocess.run([CLI, "--nominal", "--cpp", str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2   # variant A keeps the reference rule
