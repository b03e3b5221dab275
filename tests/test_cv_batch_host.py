"""Host side of the device CV (mvtv_cv_batch, multivartv_amd/csrc/mvtv_cv.hip). No GPU.

1. The numpy transcription of k_fold_sums' index logic (cv_batch_cases.fold_sums_model: stable argsort by node, each
   run walked left to right, the member's own fold skipped) equals np.bincount on the member's training subset bit for
   bit, for W and O^T y, also where the runs interleave +-1e16 with 1 and a left-to-right sum differs from the exact
   one (as in tests/test_gpu_scatter.py).
2. The selection precondition of tests/test_gpu_cv_batch.py on the oracle alone: for every (mesh, folds) case the two
   smallest CV values of mvtv_oracle.mbs_impl_rcpp differ by >= 1e-5 relative, where the GPU comparisons are at 1e-7.
"""
import math

import numpy as np
import pytest

import cv_batch_cases as K


def _bincount_members(node, y, fold, N, members):
    W = np.zeros((members, N))
    oty = np.zeros((members, N))
    for b in range(members):
        tr = np.ones(node.size, dtype=bool) if b == 0 else fold != b - 1
        W[b] = np.bincount(node[tr], minlength=N).astype(np.float64)
        oty[b] = np.bincount(node[tr], weights=y[tr], minlength=N)
    return W, oty


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("seed,n,N,folds", [(0, 100, 20, 5), (1, 300, 64, 2), (2, 40, 8, 40), (3, 257, 5, 3)])
def test_fold_sums_model_is_bincount_on_the_training_subset(seed, n, N, folds):
    rng = np.random.default_rng(seed)
    node = rng.integers(0, N, n)
    y = rng.standard_normal(n)
    fold = rng.permutation(n) % folds
    W, oty = K.fold_sums_model(node, y, fold, N, 1 + folds)
    Wr, otyr = _bincount_members(node, y, fold, N, 1 + folds)
    assert _same_bits(W, Wr) and _same_bits(oty, otyr)


def test_fold_sums_model_without_folds():
    rng = np.random.default_rng(9)
    node = rng.integers(0, 12, 50)
    y = rng.standard_normal(50)
    W, oty = K.fold_sums_model(node, y, None, 12, 1)
    assert _same_bits(W[0], np.bincount(node, minlength=12).astype(np.float64))
    assert _same_bits(oty[0], np.bincount(node, weights=y, minlength=12))


def test_fold_sums_model_on_the_adversarial_runs():
    """+-1e16 and 1 interleaved inside the runs: the model is bincount's left-to-right sum, not the exact one."""
    _, _, y, fold, node = K.adversarial()
    members, N = 4, 20
    W, oty = K.fold_sums_model(node, y, fold, N, members)
    Wr, otyr = _bincount_members(node, y, fold, N, members)
    assert _same_bits(W, Wr) and _same_bits(oty, otyr)
    # the data set is what the GPU test says it is
    assert W[0, 3] == 300 and W[2, 7] == 0 and W[0, 7] == 40 and W[1, 7] == 40 and W[3, 7] == 40
    assert all(W[0, k] == 0 for k in (0, 5, 11, 12, 19))
    exact = math.fsum(y[node == 3])
    assert oty[0, 3] != exact   # order matters here: 1e16 absorbs the 1 that follows it


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_oracle_selection_gap(case):
    gap = K.cv_gap(K.oracle(case)["cv_mses"])
    print(f"{K.case_id(case)}: relative gap between the two smallest CV values {gap:.2e}")
    assert gap >= 1e-5
