"""The fused edge passes (k_admm3a, k_admm4a + k_gather4b, k_admm2d of mvtv_admm3d.hip) under every ADMM variant, on
meshes of more than one tile, against independent CPU loops; and a table that proves from the launch log that every
instantiation a release build can reach ran in one of these checked cases ("fused edge passes").

Template arguments as the launch log prints them: k_admm3a / k_admm4a<ORD, UM, DTH, NB, TW>, k_admm2d<ORD, UM, DTH, NB>,
k_gather4b<UM, PREV>. ORD 0 = C++ block order, 1 = Python's; UM 0 = u explicit in the edge buffer (the first iteration
of a run from a caller's or the variant's default u), 1 = u read from z (every later one); DTH = the per-node
max|theta - theta_old| reduction, the only stopping test of variants A and C; NB = blocks of D (the Python order with
deltas drops the all-ones block); TW = twin blocks skipped (equal twin weights and equal twin state).

References. Variants A and C: oracle/variants_spectral.py (the statements of cpp-code/solvers.cpp:90-130 and
code/solvers.py:53-76 over the C oracle's matrix-free D / D^T and scipy.fft's exact solve; pinned on the CPU against the
SuperLU loops and the reference's own outputs in test_oracle_variants.py). Variant B (the DTH = false instantiations):
the C oracle's loop, as test_gpu_fused3d.py.

Bounds (the project's, test_gpu_fused3d.py / test_gpu_parity.py): iterations and rho exactly; theta to 1e-9 of
max|theta_ref|; u to 1e-9 of max(1, max|u_ref|); stats["dtheta_max"] to 1e-9 relative of the reference's last
max|theta - theta_old| (absolute floor 1e-12: a converged variant-A run ends at exactly 0); for A r_norm and s_norm to
1e-9 relative (absolute 1e-14). Before a GPU result is compared, the reference alone must show that no decision of
the run sits within 1e-6 (relative) of its threshold: every |dtheta / tol - 1| and, for A, r_norm / s_norm against 20
and 1 / 20. An iteration count is then a property of the algorithm, not of rounding.

Meshes: [72, 72, 24] (k_admm3a: 64 x 14 tiles, ragged in x and y, 2 x 6 tiles; the launch's chunking gives a workgroup
more than one plane and the mesh more than one chunk, so chunk-start planes are recomputed and sums carried: asserted
from the logged grid); [130, 40] (k_admm2d: three 63-column tiles, the last ragged); [65, 65, 65, 3] (k_admm4a: ragged
64-column tiles, several w; fixed iterations, its reference costs about a second per iteration); [13, 13, 13, 6]
(k_admm4a: every plane a chunk; the converged 4-D runs); [65, 65, 4] with W != I (the host-synchronous loop: the same
kernels without a control block, rho and the thresholds passed by value, under the cosine-preconditioned PCG).

Instantiations no release build reaches, and so without a case: k_gather4b<0, true> and k_gather4b<1, false> (every
gather of an explicit u is the run's first and has no previous D^T u; every gather from z has one).
"""
import functools

import numpy as np
import pytest

from conftest import log_parity

mv = pytest.importorskip("multivartv_amd")
c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd._lib import launch_log  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402
from oracle import variants_spectral as V  # noqa: E402

gpu = pytest.mark.gpu

M3, M2, M4, M4R, MW = (72, 72, 24), (130, 40), (13, 13, 13, 6), (65, 65, 65, 3), (65, 65, 4)
UNEQ = (0.3, 0.5, 0.7, 0.9)       # delta_0 != delta_1 (!= delta_2): the twin blocks carry different weights
MARGIN = 1e-6
FUSED = ("k_admm3a<", "k_admm4a<", "k_admm2d<", "k_gather4b<")
BLOCK = {"k_admm3a": {True: 1024, False: 1024}, "k_admm4a": {True: 768, False: 512}, "k_admm2d": {False: 256}}


def case(variant, m, lam, order="cpp", weighted=True, uneq=False, u0=False, fixed=None, tol=None, wmask=False):
    """One run. uneq: the deltas of UNEQ instead of (1 + 2e-4) / m_j; u0: an explicit u whose twin blocks differ."""
    return dict(variant=variant, m=m, lam=lam, order=order, weighted=weighted, uneq=uneq, u0=u0, fixed=fixed, tol=tol,
                wmask=wmask)


LAYOUTS = [dict(order="cpp", weighted=True), dict(order="py", weighted=True), dict(order="py", weighted=False)]
# twins differing: by weight where the blocks are weighted, by state (an explicit u0) where all weights are 1
NO_TWIN = [dict(order="cpp", weighted=True, uneq=True), dict(order="py", weighted=True, uneq=True),
           dict(order="py", weighted=False, u0=True)]

CASES = (
    # ---- variant A: rho 300 -> 30 -> 3 -> 0, 30 -> 3 -> 0, and 2 -> 0; the threshold at rho = 0 is +inf
    [case("A", m, lam) for m in (M3, M2) for lam in (300.0, 30.0, 2.0)]
    # rho still non-zero and just changed: dtheta_max, theta and u after 1 .. 4 iterations (the c_prev rescale of u
    # read from z)
    + [case("A", m, 300.0, fixed=k) for m in (M3, M2) for k in (1, 2, 3, 4)]
    + [case("A", M4R, 30.0, fixed=4), case("A", M4, 30.0)]
    # ---- variant C at tol = 1e-2 (27 .. 39 iterations)
    + [case("C", M3, 2.0, tol=1e-2), case("C", M3, 2.0, order="py", weighted=False, tol=1e-2),
       case("C", M2, 2.0, order="py", weighted=False, tol=1e-2), case("C", M4, 2.0, order="py", tol=1e-2)]
    # ---- the remaining block orders with DTH, twins skipped and not
    + [case("A", M3, 30.0, order="py"), case("A", M2, 30.0, order="py"),
       case("A", M4, 30.0, order="py", weighted=False)]
    + [case("A", m, 30.0, **kw) for m in (M3, M4) for kw in NO_TWIN]
    # ---- W != I: the host-synchronous loop
    + [case("A", MW, 30.0, wmask=True)]
    # ---- variant B, 4 fixed iterations: the DTH = false instantiations
    + [case("B", m, 1.0, fixed=4, **kw) for m in (M3, M4) for kw in LAYOUTS + NO_TWIN]
    + [case("B", M2, 1.0, fixed=4, **kw) for kw in LAYOUTS]
)


def case_id(c):
    s = f"{c['variant']}-{'x'.join(map(str, c['m']))}-lam{c['lam']:g}-{c['order']}{'' if c['weighted'] else '_unit'}"
    for key, tag in (("uneq", "uneq_deltas"), ("u0", "u0_twins_differ"), ("wmask", "W")):
        if c[key]:
            s += "-" + tag
    if c["fixed"]:
        s += f"-fixed{c['fixed']}"
    return s


def geometry(c):
    """(ORD, NB, TW) of the case, from the block layout rules alone."""
    p = len(c["m"])
    nb = (1 << p) - 1 - (1 if (c["order"] == "py" and c["weighted"]) else 0)
    tw = p >= 3 and not c["u0"] and not (c["weighted"] and c["uneq"])
    return (0 if c["order"] == "cpp" else 1), nb, tw


def expected_kernels(c, iters):
    """{kernel name: block size}: the fused instantiations the run must launch (and no other fused one)."""
    p = len(c["m"])
    o, nb, tw = geometry(c)
    dth = "false" if c["variant"] == "B" else "true"
    ums = (0, 1) if iters >= 2 else (0,)
    out = {}
    for um in ums:
        if p == 2:
            out[f"k_admm2d<{o}, {um}, {dth}, {nb}>"] = BLOCK["k_admm2d"][False]
        else:
            k = "k_admm3a" if p == 3 else "k_admm4a"
            out[f"{k}<{o}, {um}, {dth}, {nb}, {'true' if tw else 'false'}>"] = BLOCK[k][tw]
    if p == 4:
        out["k_gather4b<0, false>"] = 256   # D^T u0 of the explicit initial u
        out["k_gather4b<1, true>"] = 256
    return out


# every instantiation a release build can reach (launch_admm3d / launch_admm2d / launch_admm4a / launch_gather4 pick
# among exactly these; the two k_gather4b instantiations left out are named in the module docstring)
REACHABLE = (
    [f"k_admm3a<{o}, {um}, {d}, {nb}, {t}>" for o, nb in ((0, 7), (1, 6), (1, 7)) for um in (0, 1)
     for d in ("true", "false") for t in ("true", "false")]
    + [f"k_admm4a<{o}, {um}, {d}, {nb}, {t}>" for o, nb in ((0, 15), (1, 14), (1, 15)) for um in (0, 1)
       for d in ("true", "false") for t in ("true", "false")]
    + [f"k_admm2d<{o}, {um}, {d}, {nb}>" for o, nb in ((0, 3), (1, 2), (1, 3)) for um in (0, 1)
       for d in ("true", "false")]
    + ["k_gather4b<0, false>", "k_gather4b<1, true>"]
)


def test_every_reachable_instantiation_has_a_case():
    """The union of the instantiations the cases below must launch (each case asserts its own set against the launch
    log) is the whole list: 24 of k_admm3a, 24 of k_admm4a, 12 of k_admm2d, 2 of k_gather4b."""
    assert [sum(n.startswith(k) for n in REACHABLE) for k in FUSED] == [24, 24, 12, 2]
    assert len(set(REACHABLE)) == len(REACHABLE)
    covered = set()
    for c in CASES:
        # a fixed-iteration run reaches UM = 1 from its second iteration on; every converged case takes at least two
        # (asserted on its reference, test_variant_through_fused_kernels)
        covered |= set(expected_kernels(c, c["fixed"] or 2))
    assert covered == set(REACHABLE), sorted(set(REACHABLE) - covered) + sorted(covered - set(REACHABLE))
    assert len({case_id(c) for c in CASES}) == len(CASES)


def _deltas(c):
    m = c["m"]
    return list(UNEQ[:len(m)]) if c["uneq"] else [(1.0 + 2e-4) / v for v in m]


@functools.lru_cache(maxsize=None)
def _data(m, wmask):
    y = towers(list(m))
    if not wmask:
        return y, None, float(y.mean())
    W = (np.random.default_rng(len(m)).permutation(y.size) % 5 < 3).astype(float)   # 3 in 5 nodes observed
    return W * y, W, float((W * y).sum() / W.sum())


def _u0(c, E):
    """The variant's default u plus noise: every block differs from its twin."""
    base = 0.0 if c["variant"] == "B" else 1.0 / c["lam"]
    return base + 0.05 * np.random.default_rng(7).standard_normal(E)


def _superlu_solve(c, W):
    """solve(sigma, b) of (diag W + sigma D^T D) x = b from the explicit D (W != I: no cosine basis)."""
    from scipy.sparse import diags
    from scipy.sparse.linalg import splu
    from oracle import mvtv_oracle as O
    m = list(c["m"])
    D = O.build_D(m, O.block_table(len(m), _deltas(c), c["order"], unit_weights=not c["weighted"]))
    crossD = (D.T @ D).tocsc()
    lu = {}

    def solve(sigma, b):
        if sigma not in lu:
            lu[sigma] = splu((diags(W) + sigma * crossD).tocsc())
        return lu[sigma].solve(b)

    return solve


def _reference(c, oty, W, ymean, th0, u0):
    """(theta, u, rho, iters, last history entry or None) of the CPU loop; for A and C the margins are asserted."""
    m, lam = list(c["m"]), c["lam"]
    deltas = _deltas(c)
    if c["variant"] == "B":
        th, u = th0.copy(), (np.zeros(c_oracle.num_edges(m, *_codes(c))) if u0 is None else u0.copy())
        rs = c_oracle.admm_rcpp(m, oty, lam, th, u, lam / 5, deltas, order=_codes(c)[0], weighted=_codes(c)[1],
                                fixed_iters=c["fixed"], pcg_rtol=1e-13)
        return th, u, rs["rho"], rs["iters"], None
    kw = dict(order=c["order"], weighted=c["weighted"], fixed_iters=c["fixed"], u0=u0,
              solve=None if W is None else _superlu_solve(c, W))
    if c["tol"] is not None:
        kw["tol"] = c["tol"]
    fn = V.admm_cpp_spectral if c["variant"] == "A" else V.admm_py_spectral
    res = fn(m, oty, lam, th0, ymean, deltas, **kw)
    # conditions on the reference alone: no decision of this run is a matter of rounding
    if c["fixed"] is None:
        assert len(res.stop_margins) == res.iters + 1 and res.iters >= 2
        assert min(res.stop_margins) >= MARGIN, res.stop_margins
    if c["variant"] == "A":
        assert min(min(h["adapt_hi"], h["adapt_lo"]) for h in res.history) >= MARGIN, res.history
    return res.theta, res.u, res.rho, res.iters, res.history[-1]


def _codes(c):
    return (0 if c["order"] == "cpp" else 1), (1 if c["weighted"] else 0)


def _close(got, ref, rel, floor):
    return abs(got - ref) <= max(rel * abs(ref), floor)


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_variant_through_fused_kernels(c):
    m, lam = list(c["m"]), c["lam"]
    oty, W, ymean = _data(c["m"], c["wmask"])
    th0 = np.full(oty.size, ymean)
    E = c_oracle.num_edges(m, *_codes(c))
    u0 = _u0(c, E) if c["u0"] else None
    ref_th, ref_u, ref_rho, ref_iters, last = _reference(c, oty, W, ymean, th0, u0)

    variant = {"A": mv.VARIANT_CPP, "B": mv.VARIANT_RCPP, "C": mv.VARIANT_PY}[c["variant"]]
    opts = dict(pcg_rtol=1e-13)
    if c["fixed"]:
        opts["fixed_iters"] = c["fixed"]
    if c["tol"] is not None:
        opts["tol"] = c["tol"]
    if c["variant"] == "B":
        u_in, rho_in = (np.zeros(E) if u0 is None else u0), lam / 5
    else:
        u_in, rho_in, opts["ymean"] = u0, None, ymean
    with mv.Problem(m, oty, wdiag=W, deltas=_deltas(c), order=mv.ORDER_CPP if c["order"] == "cpp" else mv.ORDER_PY,
                    weighted=c["weighted"]) as P:
        assert P.E == E
        with launch_log() as log:
            th, u, rho, st = P.admm(lam, th0, u=u_in, rho=rho_in, variant=variant, **opts)
    assert st["theta_solver"] == (mv.SOLVER_SPECTRAL if W is None else mv.SOLVER_PCG_SPECTRAL)
    assert st["pcg_unconverged"] == 0

    # ---- the launch log: exactly this case's fused instantiations, at their block sizes
    assert log and not log[0][0].startswith("#"), log[:1]
    fused = [(n, g, b) for n, g, b in log if n.startswith(FUSED)]
    expect = expected_kernels(c, ref_iters)
    assert {n for n, _, _ in fused} == set(expect), (sorted({n for n, _, _ in fused}), sorted(expect))
    for n, g, b in fused:
        assert b == (expect[n], 1, 1) and g[1:] == (1, 1) and g[0] % 8 == 0, (n, g, b)
    grids = sorted({g[0] for n, g, _ in fused if not n.startswith("k_gather4b")})
    assert len(grids) == 1, grids
    if c["m"] == M3:
        # 2 x 6 tiles a plane: more than one chunk of more than one plane (a chunk start is recomputed, sums are carried)
        assert 12 < grids[0] < 12 * 24, grids

    # ---- the run against the reference
    assert st["iters"] == ref_iters
    assert rho == ref_rho and st["rho"] == ref_rho
    e_th = float(np.max(np.abs(th - ref_th)) / np.max(np.abs(ref_th)))
    e_u = float(np.max(np.abs(u - ref_u)) / max(1.0, np.max(np.abs(ref_u))))
    rec = dict(theta=e_th, u=e_u, iters=int(ref_iters), rho=float(ref_rho), grid=int(grids[0]),
               kernels=" | ".join(sorted(expect)))
    if last is not None:
        rec.update(dtheta_ref=last["dtheta_max"], dtheta_err=abs(st["dtheta_max"] - last["dtheta_max"]))
        if c["variant"] == "A":
            rec.update(r_err=abs(st["r_norm"] - last["r_norm"]) / max(last["r_norm"], 1e-300),
                       s_err=abs(st["s_norm"] - last["s_norm"]) / max(last["s_norm"], 1e-300) if last["s_norm"] else
                       abs(st["s_norm"]))
    print(case_id(c), rec)
    log_parity("fused " + case_id(c), **rec)
    assert e_th <= 1e-9
    assert e_u <= 1e-9
    if last is not None:
        assert _close(st["dtheta_max"], last["dtheta_max"], 1e-9, 1e-12), (st["dtheta_max"], last["dtheta_max"])
        if c["variant"] == "A":
            assert _close(st["r_norm"], last["r_norm"], 1e-9, 1e-14), (st["r_norm"], last["r_norm"])
            assert _close(st["s_norm"], last["s_norm"], 1e-9, 1e-14), (st["s_norm"], last["s_norm"])
