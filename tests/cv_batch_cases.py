"""Shared by tests/test_cv_batch_host.py and tests/test_gpu_cv_batch.py: the (mesh, n, folds) cases of the device CV
(mvtv_cv_batch), their data and fold labels, the oracle's result per case (computed once per process) and the numpy
transcription of k_fold_sums (multivartv_amd/csrc/mvtv_cv.hip)."""
import functools

import numpy as np

import small_batch_cases as S
from multivartv_amd import cv
from oracle import mvtv_oracle as O

LAMS = S.LAMS
FOLD_SEED = 11

# (m, n, folds); the last is leave-one-out: every fold has a single test point
CASES = [(m, n, f) for m, n in (([20], 100), ([10, 10], 100), ([4, 4, 4], 300), ([3, 3, 3, 3], 400)) for f in (1, 2, 5)]
CASES.append(([8], 40, 40))


def case_id(c):
    m, n, folds = c
    return "x".join(str(v) for v in m) + f"-n{n}-f{folds}"


def scattered(n, p, seed=0):
    """_scattered of tests/test_gpu_small_batch_cv.py."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(n, p))
    f = np.where(np.all(x > 0.6, axis=1), 1.0, 0.0)
    return x, f + 0.3 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _data(m, n, folds):
    x, y = scattered(n, len(m), seed=10 * len(m) + folds)
    fi = cv.kfoldinds(n, folds, FOLD_SEED) if folds > 1 else None
    return x, y, fi


def data(c):
    """(x, y, fold labels or None) of a case."""
    m, n, folds = c
    return _data(tuple(m), n, folds)


@functools.lru_cache(maxsize=None)
def _oracle(m, n, folds):
    x, y, fi = _data(m, n, folds)
    return O.mbs_impl_rcpp(x, y, list(m), LAMS, foldinds=fi, folds=folds)


def oracle(c):
    m, n, folds = c
    return _oracle(tuple(m), n, folds)


def cv_gap(cv_mses):
    """Relative gap between the two smallest CV values."""
    v = np.sort(np.asarray(cv_mses, dtype=np.float64))
    return float((v[1] - v[0]) / v[0])


def fold_sums_model(node, y, fold, N, members):
    """k_fold_sums' index logic: the (node, position) pairs sorted stably by node; the first element of each run of
    equal nodes walks the run left to right once per member, skips the points of the member's own fold (member b >= 1
    tests fold b - 1) and adds y into the member's O^T y and 1 into its W. Returns (W, O^T y), each [members][N]."""
    node = np.asarray(node, dtype=np.int64)
    n = node.size
    pos = np.argsort(node, kind="stable")
    key = node[pos]
    W = np.zeros((members, N))
    oty = np.zeros((members, N))
    for i in range(n):
        k = key[i]
        if i > 0 and key[i - 1] == k:
            continue
        for b in range(members):
            s, cnt, j = np.float64(0.0), 0, i
            while j < n and key[j] == k:
                q = pos[j]
                j += 1
                if b > 0 and fold[q] == b - 1:
                    continue
                s = s + np.float64(y[q])
                cnt += 1
            oty[b, k] = s
            W[b, k] = float(cnt)
    return W, oty


def adversarial():
    """1-D m = 20, n = 700, three folds: node 3 holds 300 points (a run that crosses 256-thread workgroups), node 7's
    points all lie in fold 1 (member 2's W is 0 there, the others' is not), nodes 0, 5, 11, 12 and 19 are empty, and
    inside the runs y interleaves +-1e16 with 1, where a left-to-right sum differs from the exact one.
    Returns (axes, x, y, fold, node)."""
    rng = np.random.default_rng(5)
    n, m = 700, 20
    node = np.empty(n, dtype=np.int64)
    node[:300] = 3
    node[300:340] = 7
    rest = np.array([v for v in range(m) if v not in (0, 3, 5, 7, 11, 12, 19)])
    node[340:] = rest[rng.integers(0, rest.size, n - 340)]
    perm = rng.permutation(n)
    node = node[perm]
    fold = rng.integers(0, 3, n).astype(np.int64)
    fold[node == 7] = 1
    pattern = np.array([1e16, 1.0, -1e16, 1.0])
    y = np.empty(n)
    for k in range(m):   # the pattern runs along each node's points in data order
        at = np.flatnonzero(node == k)
        y[at] = pattern[np.arange(at.size) % 4]
    y[node == 14] = 0.5 + 0.1 * rng.standard_normal(int(np.sum(node == 14)))   # one ordinary node
    x = (node + rng.uniform(-0.3, 0.3, n)).reshape(-1, 1)
    return [np.arange(m, dtype=np.float64)], x, y, fold, node
