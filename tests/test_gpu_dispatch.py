"""Every default spectral-solve kernel tile, run in a checked test ("Dispatch coverage").

The launchers of mvtv_spectral.hip choose between some 280 template instantiations by line length, line count, stride
and pass mode. Each case below carries a mesh, the launch log one ``solve_spectral`` on it must produce (kernel name
with template arguments, grid, block: ``multivartv_amd._lib.launch_log``) and a forward-error check of the result
against the long-double cosine-transform reference (oracle/spectral_ld.py). A case fails when the log differs, so
a later change of a dispatch heuristic cannot silently un-test a tile: it has to move the tile's case with it.

Template arguments as the log prints them: k_dct8<L, mode, d0, formb, lines per workgroup, pcg fuse>, mode 0 FWD, 1 INV,
2 MID (forward, divide, inverse); k_dctb8<L = log2 M, mode, d0, formb, lines>; k_dctm<m, mode, d0, formb, line pairs>;
k_dctg / k_dct<mode, d0, formb>; k_plane8<L, mode, formb>; k_trir<L, rows per segment, lines>; k_trigr<max rows per
segment, lines, max segments>. A grid of None is a persistent launch sized by the CU count (k_plane8<7>).
The narrow-stride fallback of launch_dct8 (a stride of 2 / 4 / 8 below the smallest tile tile_ok<L> allows) runs the
default tile's instantiation k_dct8<L, .., 16, 0> with 2 / 4 / 8 lines: its cases are 2 x {8 ... 256}, 4 x {8 ... 128}
and 8 x {8 ... 64} (one workgroup each, so the log shows the instantiation and the stride leaves no other tile) and
8 x 8 x 11, 8^4 (told by their grids). From 2 x 512, 4 x 256 and 8 x 128 on the 2- / 4- / 8-line instantiations run.

Bound (per case and sigma): e64 = max|x64 - x_ld| / max|x_ld| is the error of a float64 pocketfft evaluation of the same
formula, a property of the reference alone (0.6e-15 ... 2e-15 on a CPU). The GPU must satisfy
max|x_gpu - x_ld| <= min(1e-12, K e64) max|x_ld| with K = 32: the factorised line solve sits at 3e-14 against a
long-double Thomas solve at c1 / c0 = 1e7 where well-conditioned lines sit at 1e-15, a factor of
about 30 that belongs to the algorithm. b = randn + 2: the mean passes through the solve unchanged, so max|x_ld| is
at least |mean b|, about 2, at every sigma and a relative bound is meaningful.

The instantiations no release build could reach (probe_env only: the Thomas-form line solves, k_dctb, k_march, the
forced k_trir tiles, k_dctm<.., 8>) had no case and were removed from the library.
Release-reachable ones without a case are listed in DESIGN.md §2 with the reason (they need more than 2^24 nodes, or
a CPU reference run of tens of seconds).
"""
import functools
import os

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

K_BOUND = 32.0
RTOL_DIRECT = 1e-12
SIGMAS = (0.0, 1e-3, 3.7, 2e5)
SIGMAS_BIG = (1e-3, 2e5)          # above 2^23 nodes: the long-double transforms cost seconds each
WORKERS = min(16, os.cpu_count() or 1)

# (mesh, [(kernel, grid, block) of one solve_spectral, in launch order])
DISPATCH = [
    # 32-row segments with a shorter last one (2039 = 63 x 32 + 23) on the few-lines tile
    ([1024, 2039], [("k_dct8<10, 0, true, false, 2, 0>", 1020, 128), ("k_trigr<32, 4, 64>", 256, 256),
     ("k_dct8<10, 1, true, false, 2, 0>", 1020, 128)]),
    ([2], [("k_dct<2, true, false>", 1, 256)]),
    ([3], [("k_dctg<2, true, false>", 1, 512)]),
    ([4], [("k_dct<2, true, false>", 1, 256)]),
    ([8], [("k_dct8<3, 2, true, false, 16, 0>", 1, 8)]),
    ([13], [("k_dctb8<5, 2, true, false, 32>", 1, 64)]),
    ([16], [("k_dct8<4, 2, true, false, 16, 0>", 1, 16)]),
    ([31], [("k_dctb8<6, 2, true, false, 16>", 1, 64)]),
    ([32], [("k_dct8<5, 2, true, false, 16, 0>", 1, 32)]),
    ([37], [("k_dctb8<7, 2, true, false, 16>", 1, 128)]),
    ([64], [("k_dct8<6, 2, true, false, 16, 0>", 1, 64)]),
    ([67], [("k_dctb8<8, 2, true, false, 16>", 1, 256)]),
    ([128], [("k_dct8<7, 2, true, false, 8, 0>", 1, 64)]),
    ([251], [("k_dctb8<9, 2, true, false, 2>", 1, 64)]),
    ([256], [("k_dct8<8, 2, true, false, 4, 0>", 1, 64)]),
    ([509], [("k_dctb8<10, 2, true, false, 2>", 1, 128)]),
    ([512], [("k_dct8<9, 2, true, false, 2, 0>", 1, 64)]),
    ([1009], [("k_dctb8<11, 2, true, false, 4>", 1, 512)]),
    ([1024], [("k_dct8<10, 2, true, false, 2, 0>", 1, 128)]),
    ([2039], [("k_dctb8<12, 2, true, false, 2>", 1, 512)]),
    ([2048], [("k_dct8<11, 2, true, false, 2, 0>", 1, 256)]),
    ([4093], [("k_dctb8<13, 2, true, false, 2>", 1, 1024)]),
    ([4096], [("k_dct8<12, 2, true, false, 2, 0>", 1, 512)]),
    ([2, 2], [("k_dct<0, true, false>", 1, 256), ("k_dct<2, false, false>", 1, 256),
         ("k_dct<1, true, false>", 1, 256)]),
    ([2, 8], [("k_dct<0, true, false>", 1, 256), ("k_dct8<3, 2, false, false, 16, 0>", 1, 8),
         ("k_dct<1, true, false>", 1, 256)]),
    ([2, 16], [("k_dct<0, true, false>", 1, 256), ("k_dct8<4, 2, false, false, 16, 0>", 1, 16),
         ("k_dct<1, true, false>", 1, 256)]),
    ([4, 8], [("k_dct<0, true, false>", 1, 256), ("k_dct8<3, 2, false, false, 16, 0>", 1, 8),
         ("k_dct<1, true, false>", 1, 256)]),
    ([2, 32], [("k_dct<0, true, false>", 2, 256), ("k_dct8<5, 2, false, false, 16, 0>", 1, 32),
         ("k_dct<1, true, false>", 2, 256)]),
    ([4, 16], [("k_dct<0, true, false>", 1, 256), ("k_dct8<4, 2, false, false, 16, 0>", 1, 16),
         ("k_dct<1, true, false>", 1, 256)]),
    ([8, 8], [("k_dct8<3, 0, true, false, 16, 0>", 1, 8), ("k_dct8<3, 2, false, false, 16, 0>", 1, 8),
         ("k_dct8<3, 1, true, false, 16, 0>", 1, 8)]),
    ([2, 64], [("k_dct<0, true, false>", 4, 256), ("k_dct8<6, 2, false, false, 16, 0>", 1, 64),
         ("k_dct<1, true, false>", 4, 256)]),
    ([4, 32], [("k_dct<0, true, false>", 2, 256), ("k_dct8<5, 2, false, false, 16, 0>", 1, 32),
         ("k_dct<1, true, false>", 2, 256)]),
    ([8, 16], [("k_dct8<3, 0, true, false, 16, 0>", 1, 8), ("k_dct8<4, 2, false, false, 16, 0>", 1, 16),
         ("k_dct8<3, 1, true, false, 16, 0>", 1, 8)]),
    ([64, 2], [("k_dct8<6, 0, true, false, 16, 0>", 1, 64), ("k_dct<2, false, false>", 4, 256),
         ("k_dct8<6, 1, true, false, 16, 0>", 1, 64)]),
    ([8, 31], [("k_dct8<3, 0, true, false, 16, 0>", 2, 8), ("k_dctb8<6, 2, false, false, 16>", 1, 64),
         ("k_dct8<3, 1, true, false, 16, 0>", 2, 8)]),
    ([2, 128], [("k_dct<0, true, false>", 8, 256), ("k_dct8<7, 2, false, false, 16, 0>", 1, 128),
         ("k_dct<1, true, false>", 8, 256)]),
    ([4, 64], [("k_dct<0, true, false>", 4, 256), ("k_dct8<6, 2, false, false, 16, 0>", 1, 64),
         ("k_dct<1, true, false>", 4, 256)]),
    ([8, 32], [("k_dct8<3, 0, true, false, 16, 0>", 2, 8), ("k_dct8<5, 2, false, false, 16, 0>", 1, 32),
         ("k_dct8<3, 1, true, false, 16, 0>", 2, 8)]),
    ([16, 16], [("k_dct8<4, 0, true, false, 16, 0>", 1, 16), ("k_dct8<4, 2, false, false, 16, 0>", 1, 16),
         ("k_dct8<4, 1, true, false, 16, 0>", 1, 16)]),
    ([128, 2], [("k_dct8<7, 0, true, false, 8, 0>", 1, 64), ("k_dct<2, false, false>", 8, 256),
         ("k_dct8<7, 1, true, false, 8, 0>", 1, 64)]),
    ([8, 37], [("k_dct8<3, 0, true, false, 16, 0>", 3, 8), ("k_dctb8<7, 2, false, false, 16>", 1, 128),
         ("k_dct8<3, 1, true, false, 16, 0>", 3, 8)]),
    ([16, 24], [("k_dct8<4, 0, true, false, 16, 0>", 2, 16), ("k_dctg<2, false, false>", 8, 512),
         ("k_dct8<4, 1, true, false, 16, 0>", 2, 16)]),
    ([251, 2], [("k_dctb8<9, 0, true, false, 2>", 1, 64), ("k_dctg<2, false, false>", 126, 512),
         ("k_dctb8<9, 1, true, false, 2>", 1, 64)]),
    ([2, 256], [("k_dct<0, true, false>", 16, 256), ("k_dct8<8, 2, false, false, 16, 0>", 1, 256),
         ("k_dct<1, true, false>", 16, 256)]),
    ([4, 128], [("k_dct<0, true, false>", 8, 256), ("k_dct8<7, 2, false, false, 16, 0>", 1, 128),
         ("k_dct<1, true, false>", 8, 256)]),
    ([8, 64], [("k_dct8<3, 0, true, false, 16, 0>", 4, 8), ("k_dct8<6, 2, false, false, 16, 0>", 1, 64),
         ("k_dct8<3, 1, true, false, 16, 0>", 4, 8)]),
    ([16, 32], [("k_dct8<4, 0, true, false, 16, 0>", 2, 16), ("k_dct8<5, 2, false, false, 16, 0>", 1, 32),
         ("k_dct8<4, 1, true, false, 16, 0>", 2, 16)]),
    ([32, 16], [("k_dct8<5, 0, true, false, 16, 0>", 1, 32), ("k_dct8<4, 2, false, false, 16, 0>", 2, 16),
         ("k_dct8<5, 1, true, false, 16, 0>", 1, 32)]),
    ([256, 2], [("k_dct8<8, 0, true, false, 4, 0>", 1, 64), ("k_dct<2, false, false>", 16, 256),
         ("k_dct8<8, 1, true, false, 4, 0>", 1, 64)]),
    ([8, 67], [("k_dct8<3, 0, true, false, 16, 0>", 5, 8), ("k_dctb8<8, 2, false, false, 16>", 1, 256),
         ("k_dct8<3, 1, true, false, 16, 0>", 5, 8)]),
    ([32, 24], [("k_dct8<5, 0, true, false, 16, 0>", 2, 32), ("k_dctg<2, false, false>", 16, 512),
         ("k_dct8<5, 1, true, false, 16, 0>", 2, 32)]),
    ([32, 31], [("k_dct8<5, 0, true, false, 16, 0>", 2, 32), ("k_dctb8<6, 2, false, false, 16>", 2, 64),
         ("k_dct8<5, 1, true, false, 16, 0>", 2, 32)]),
    ([500, 2], [("k_dctm<500, 0, true, false, 1>", 1, 50), ("k_dctg<2, false, false>", 250, 512),
         ("k_dctm<500, 1, true, false, 1>", 1, 50)]),
    ([2, 509], [("k_dct<0, true, false>", 32, 256), ("k_dctb8<10, 2, false, false, 2>", 1, 128),
         ("k_dct<1, true, false>", 32, 256)]),
    ([509, 2], [("k_dctb8<10, 0, true, false, 2>", 1, 128), ("k_dctg<2, false, false>", 255, 512),
         ("k_dctb8<10, 1, true, false, 2>", 1, 128)]),
    ([2, 512], [("k_dct<0, true, false>", 32, 256), ("k_dct8<9, 2, false, false, 2, 0>", 1, 64),
         ("k_dct<1, true, false>", 32, 256)]),
    ([4, 256], [("k_dct<0, true, false>", 16, 256), ("k_dct8<8, 2, false, false, 4, 0>", 1, 64),
         ("k_dct<1, true, false>", 16, 256)]),
    ([8, 128], [("k_dct8<3, 0, true, false, 16, 0>", 8, 8), ("k_dct8<7, 2, false, false, 8, 0>", 1, 64),
         ("k_dct8<3, 1, true, false, 16, 0>", 8, 8)]),
    ([512, 2], [("k_dct8<9, 0, true, false, 2, 0>", 1, 64), ("k_dct<2, false, false>", 32, 256),
         ("k_dct8<9, 1, true, false, 2, 0>", 1, 64)]),
    ([16, 67], [("k_dct8<4, 0, true, false, 16, 0>", 5, 16), ("k_dctb8<8, 2, false, false, 16>", 1, 256),
         ("k_dct8<4, 1, true, false, 16, 0>", 5, 16)]),
    ([128, 10], [("k_dct8<7, 0, true, false, 8, 0>", 2, 64), ("k_dctg<2, false, false>", 64, 512),
         ("k_dct8<7, 1, true, false, 8, 0>", 2, 64)]),
    ([64, 24], [("k_dct8<6, 0, true, false, 16, 0>", 2, 64), ("k_dctg<2, false, false>", 32, 512),
         ("k_dct8<6, 1, true, false, 16, 0>", 2, 64)]),
    ([128, 12], [("k_dct8<7, 0, true, false, 8, 0>", 2, 64), ("k_dctg<2, false, false>", 64, 512),
         ("k_dct8<7, 1, true, false, 8, 0>", 2, 64)]),
    ([256, 6], [("k_dct8<8, 0, true, false, 4, 0>", 2, 64), ("k_dctg<2, false, false>", 128, 512),
         ("k_dct8<8, 1, true, false, 4, 0>", 2, 64)]),
    ([512, 3], [("k_dct8<9, 0, true, false, 2, 0>", 2, 64), ("k_dctg<2, false, false>", 256, 512),
         ("k_dct8<9, 1, true, false, 2, 0>", 2, 64)]),
    ([16, 100], [("k_dct8<4, 0, true, false, 16, 0>", 7, 16), ("k_dctg<2, false, false>", 8, 512),
         ("k_dct8<4, 1, true, false, 16, 0>", 7, 16)]),
    ([64, 31], [("k_dct8<6, 0, true, false, 16, 0>", 2, 64), ("k_dctb8<6, 2, false, false, 16>", 4, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 2, 64)]),
    ([1000, 2], [("k_dctm<1000, 0, true, false, 1>", 1, 50), ("k_dctg<2, false, false>", 500, 512),
         ("k_dctm<1000, 1, true, false, 1>", 1, 50)]),
    ([2, 1009], [("k_dct<0, true, false>", 64, 256), ("k_dctb8<11, 2, false, false, 4>", 1, 512),
         ("k_dct<1, true, false>", 64, 256)]),
    ([1009, 2], [("k_dctb8<11, 0, true, false, 4>", 1, 512), ("k_dctg<2, false, false>", 505, 512),
         ("k_dctb8<11, 1, true, false, 4>", 1, 512)]),
    ([2, 1024], [("k_dct<0, true, false>", 64, 256), ("k_dct8<10, 2, false, false, 2, 0>", 1, 128),
         ("k_dct<1, true, false>", 64, 256)]),
    ([4, 512], [("k_dct<0, true, false>", 32, 256), ("k_dct8<9, 2, false, false, 4, 0>", 1, 128),
         ("k_dct<1, true, false>", 32, 256)]),
    ([8, 256], [("k_dct8<3, 0, true, false, 16, 0>", 16, 8), ("k_dct8<8, 2, false, false, 8, 0>", 1, 128),
         ("k_dct8<3, 1, true, false, 16, 0>", 16, 8)]),
    ([32, 64], [("k_dct8<5, 0, true, false, 16, 0>", 4, 32), ("k_dct8<6, 2, false, false, 16, 0>", 2, 64),
         ("k_dct8<5, 1, true, false, 16, 0>", 4, 32)]),
    ([512, 4], [("k_dct8<9, 0, true, false, 2, 0>", 2, 64), ("k_dct<2, false, false>", 32, 256),
         ("k_dct8<9, 1, true, false, 2, 0>", 2, 64)]),
    ([1024, 2], [("k_dct8<10, 0, true, false, 2, 0>", 1, 128), ("k_dct<2, false, false>", 64, 256),
         ("k_dct8<10, 1, true, false, 2, 0>", 1, 128)]),
    ([32, 67], [("k_dct8<5, 0, true, false, 16, 0>", 5, 32), ("k_dctb8<8, 2, false, false, 16>", 2, 256),
         ("k_dct8<5, 1, true, false, 16, 0>", 5, 32)]),
    ([32, 100], [("k_dct8<5, 0, true, false, 16, 0>", 7, 32), ("k_dctg<2, false, false>", 16, 512),
         ("k_dct8<5, 1, true, false, 16, 0>", 7, 32)]),
    ([128, 31], [("k_dct8<7, 0, true, false, 8, 0>", 4, 64), ("k_dctb8<6, 2, false, false, 16>", 8, 64),
         ("k_dct8<7, 1, true, false, 8, 0>", 4, 64)]),
    ([16, 251], [("k_dct8<4, 0, true, false, 16, 0>", 16, 16), ("k_dctb8<9, 2, false, false, 2>", 8, 64),
         ("k_dct8<4, 1, true, false, 16, 0>", 16, 16)]),
    ([2, 2039], [("k_dct<0, true, false>", 128, 256), ("k_dctb8<12, 2, false, false, 2>", 1, 512),
         ("k_dct<1, true, false>", 128, 256)]),
    ([2039, 2], [("k_dctb8<12, 0, true, false, 2>", 1, 512), ("k_dctg<2, false, false>", 1020, 512),
         ("k_dctb8<12, 1, true, false, 2>", 1, 512)]),
    ([2, 2048], [("k_dct<0, true, false>", 128, 256), ("k_dct8<11, 2, false, false, 2, 0>", 1, 256),
         ("k_dct<1, true, false>", 128, 256)]),
    ([4, 1024], [("k_dct<0, true, false>", 64, 256), ("k_dct8<10, 2, false, false, 4, 0>", 1, 256),
         ("k_dct<1, true, false>", 64, 256)]),
    ([8, 512], [("k_dct8<3, 0, true, false, 16, 0>", 32, 8), ("k_dct8<9, 2, false, false, 8, 0>", 1, 256),
         ("k_dct8<3, 1, true, false, 16, 0>", 32, 8)]),
    ([32, 128], [("k_dct8<5, 0, true, false, 16, 0>", 8, 32), ("k_dct8<7, 2, false, false, 16, 0>", 2, 128),
         ("k_dct8<5, 1, true, false, 16, 0>", 8, 32)]),
    ([2048, 2], [("k_dct8<11, 0, true, false, 2, 0>", 1, 256), ("k_dct<2, false, false>", 128, 256),
         ("k_dct8<11, 1, true, false, 2, 0>", 1, 256)]),
    ([64, 67], [("k_dct8<6, 0, true, false, 16, 0>", 5, 64), ("k_dctb8<8, 2, false, false, 16>", 4, 256),
         ("k_dct8<6, 1, true, false, 16, 0>", 5, 64)]),
    ([64, 100], [("k_dct8<6, 0, true, false, 16, 0>", 7, 64), ("k_dctg<2, false, false>", 32, 512),
         ("k_dct8<6, 1, true, false, 16, 0>", 7, 64)]),
    ([2, 4093], [("k_dct<0, true, false>", 256, 256), ("k_dctb8<13, 2, false, false, 2>", 1, 1024),
         ("k_dct<1, true, false>", 256, 256)]),
    ([4093, 2], [("k_dctb8<13, 0, true, false, 2>", 1, 1024), ("k_dctg<2, false, false>", 512, 512),
         ("k_dctb8<13, 1, true, false, 2>", 1, 1024)]),
    ([2, 4096], [("k_dct<0, true, false>", 256, 256), ("k_dct8<12, 2, false, false, 2, 0>", 1, 512),
         ("k_dct<1, true, false>", 256, 256)]),
    ([4, 2048], [("k_dct<0, true, false>", 128, 256), ("k_dct8<11, 2, false, false, 4, 0>", 1, 512),
         ("k_dct<1, true, false>", 128, 256)]),
    ([8, 1024], [("k_dct8<3, 0, true, false, 16, 0>", 64, 8), ("k_dct8<10, 2, false, false, 8, 0>", 1, 512),
         ("k_dct8<3, 1, true, false, 16, 0>", 64, 8)]),
    ([32, 256], [("k_dct8<5, 0, true, false, 16, 0>", 16, 32), ("k_dct8<8, 2, false, false, 16, 0>", 2, 256),
         ("k_dct8<5, 1, true, false, 16, 0>", 16, 32)]),
    ([256, 32], [("k_dct8<8, 0, true, false, 4, 0>", 8, 64), ("k_dct8<5, 2, false, false, 16, 0>", 16, 32),
         ("k_dct8<8, 1, true, false, 4, 0>", 8, 64)]),
    ([4096, 2], [("k_dct8<12, 0, true, false, 2, 0>", 1, 512), ("k_dct<2, false, false>", 256, 256),
         ("k_dct8<12, 1, true, false, 2, 0>", 1, 512)]),
    ([3, 4096], [("k_dctg<0, true, false>", 512, 512), ("k_dctg<2, false, false>", 2, 512),
         ("k_dctg<1, true, false>", 512, 512)]),
    ([12, 1024], [("k_dctg<0, true, false>", 512, 512), ("k_dctg<2, false, false>", 6, 512),
         ("k_dctg<1, true, false>", 512, 512)]),
    ([4096, 3], [("k_dct8<12, 0, true, false, 2, 0>", 2, 512), ("k_dctg<2, false, false>", 512, 512),
         ("k_dct8<12, 1, true, false, 2, 0>", 2, 512)]),
    ([4, 4096], [("k_dct<0, true, false>", 256, 256), ("k_dct8<12, 2, false, false, 4, 0>", 1, 1024),
         ("k_dct<1, true, false>", 256, 256)]),
    ([8, 2048], [("k_dct8<3, 0, true, false, 16, 0>", 128, 8), ("k_dct8<11, 2, false, false, 4, 0>", 2, 512),
         ("k_dct8<3, 1, true, false, 16, 0>", 128, 8)]),
    ([32, 512], [("k_dct8<5, 0, true, false, 16, 0>", 32, 32), ("k_trir<9, 16, 4>", 8, 128),
         ("k_dct8<5, 1, true, false, 16, 0>", 32, 32)]),
    ([4093, 8], [("k_dctb8<13, 0, true, false, 2>", 4, 1024), ("k_trigr<32, 8, 64>", 512, 16),
         ("k_dctb8<13, 1, true, false, 2>", 4, 1024)]),
    ([8, 4096], [("k_dct8<3, 0, true, false, 16, 0>", 256, 8), ("k_dct8<12, 2, false, false, 4, 0>", 2, 1024),
         ("k_dct8<3, 1, true, false, 16, 0>", 256, 8)]),
    ([32, 1024], [("k_dct8<5, 0, true, false, 16, 0>", 64, 32), ("k_trir<10, 16, 4>", 8, 256),
         ("k_dct8<5, 1, true, false, 16, 0>", 64, 32)]),
    ([1024, 37], [("k_dct8<10, 0, true, false, 2, 0>", 19, 128), ("k_trigr<32, 4, 64>", 256, 16),
         ("k_dct8<10, 1, true, false, 2, 0>", 19, 128)]),
    ([1024, 48], [("k_dct8<10, 0, true, false, 2, 0>", 24, 128), ("k_trigr<32, 4, 64>", 256, 12),
         ("k_dct8<10, 1, true, false, 2, 0>", 24, 128)]),
    ([2048, 37], [("k_dct8<11, 0, true, false, 2, 0>", 19, 256), ("k_trigr<32, 4, 64>", 512, 16),
         ("k_dct8<11, 1, true, false, 2, 0>", 19, 256)]),
    ([2048, 48], [("k_dct8<11, 0, true, false, 2, 0>", 24, 256), ("k_trigr<32, 4, 64>", 512, 12),
         ("k_dct8<11, 1, true, false, 2, 0>", 24, 256)]),
    ([64, 2048], [("k_dct8<6, 0, true, false, 16, 0>", 128, 64), ("k_trir<11, 32, 8>", 8, 512),
         ("k_dct8<6, 1, true, false, 16, 0>", 128, 64)]),
    ([4093, 37], [("k_dctb8<13, 0, true, false, 2>", 19, 1024), ("k_trigr<32, 8, 64>", 512, 32),
         ("k_dctb8<13, 1, true, false, 2>", 19, 1024)]),
    ([4093, 48], [("k_dctb8<13, 0, true, false, 2>", 24, 1024), ("k_trigr<32, 8, 64>", 512, 24),
         ("k_dctb8<13, 1, true, false, 2>", 24, 1024)]),
    ([2048, 113], [("k_dct8<11, 0, true, false, 2, 0>", 57, 256), ("k_trigr<32, 4, 64>", 512, 32),
         ("k_dct8<11, 1, true, false, 2, 0>", 57, 256)]),
    ([4096, 64], [("k_dct8<12, 0, true, false, 2, 0>", 32, 512), ("k_trir<6, 16, 16>", 256, 64),
         ("k_dct8<12, 1, true, false, 2, 0>", 32, 512)]),
    ([4093, 113], [("k_dctb8<13, 0, true, false, 2>", 57, 1024), ("k_trigr<32, 8, 64>", 512, 64),
         ("k_dctb8<13, 1, true, false, 2>", 57, 1024)]),
    ([1024, 1009], [("k_dct8<10, 0, true, false, 2, 0>", 505, 128), ("k_trigr<32, 4, 64>", 256, 256),
         ("k_dct8<10, 1, true, false, 2, 0>", 505, 128)]),
    ([4096, 2048], [("k_dct8<12, 0, true, false, 2, 0>", 1024, 512), ("k_trir<11, 32, 8>", 512, 512),
         ("k_dct8<12, 1, true, false, 2, 0>", 1024, 512)]),
    ([4, 4, 2], [("k_dct<0, true, false>", 1, 256), ("k_dct<0, false, false>", 2, 256),
         ("k_dct<2, false, false>", 1, 256), ("k_dct<1, false, false>", 2, 256), ("k_dct<1, true, false>", 1, 256)]),
    ([8, 8, 11], [("k_dct8<3, 0, true, false, 16, 0>", 6, 8), ("k_dct8<3, 0, false, false, 16, 0>", 11, 8),
         ("k_dctb8<5, 2, false, false, 32>", 2, 64), ("k_dct8<3, 1, false, false, 16, 0>", 11, 8),
         ("k_dct8<3, 1, true, false, 16, 0>", 6, 8)]),
    ([13, 13, 11], [("k_dctb8<5, 0, true, false, 32>", 5, 64), ("k_dctb8<5, 0, false, false, 32>", 5, 64),
         ("k_dctb8<5, 2, false, false, 32>", 6, 64), ("k_dctb8<5, 1, false, false, 32>", 5, 64),
         ("k_dctb8<5, 1, true, false, 32>", 5, 64)]),
    ([31, 31, 2], [("k_dctb8<6, 0, true, false, 16>", 4, 64), ("k_dctb8<6, 0, false, false, 16>", 4, 64),
         ("k_dctg<2, false, false>", 481, 512), ("k_dctb8<6, 1, false, false, 16>", 4, 64),
         ("k_dctb8<6, 1, true, false, 16>", 4, 64)]),
    ([37, 37, 2], [("k_dctb8<7, 0, true, false, 16>", 5, 128), ("k_dctb8<7, 0, false, false, 16>", 5, 128),
         ("k_dctg<2, false, false>", 685, 512), ("k_dctb8<7, 1, false, false, 16>", 5, 128),
         ("k_dctb8<7, 1, true, false, 16>", 5, 128)]),
    ([4, 4, 512], [("k_dct<0, true, false>", 128, 256), ("k_dct<0, false, false>", 512, 256),
         ("k_dct8<9, 2, false, false, 16, 0>", 1, 512), ("k_dct<1, false, false>", 512, 256),
         ("k_dct<1, true, false>", 128, 256)]),
    ([67, 67, 2], [("k_dctb8<8, 0, true, false, 16>", 9, 256), ("k_dctb8<8, 0, false, false, 16>", 9, 256),
         ("k_dctg<2, false, false>", 562, 512), ("k_dctb8<8, 1, false, false, 16>", 9, 256),
         ("k_dctb8<8, 1, true, false, 16>", 9, 256)]),
    ([4, 4, 1024], [("k_dct<0, true, false>", 256, 256), ("k_dct<0, false, false>", 1024, 256),
         ("k_dct8<10, 2, false, false, 4, 0>", 4, 256), ("k_dct<1, false, false>", 1024, 256),
         ("k_dct<1, true, false>", 256, 256)]),
    ([251, 251, 2], [("k_dctb8<9, 0, true, false, 2>", 251, 64), ("k_dctb8<9, 0, false, false, 2>", 251, 64),
         ("k_dctg<2, false, false>", 3938, 512), ("k_dctb8<9, 1, false, false, 2>", 251, 64),
         ("k_dctb8<9, 1, true, false, 2>", 251, 64)]),
    ([256, 256, 2], [("k_dct8<8, 0, true, false, 4, 0>", 128, 64), ("k_dct8<8, 0, false, false, 16, 0>", 32, 256),
         ("k_dct<2, false, false>", 4096, 256), ("k_dct8<8, 1, false, false, 16, 0>", 32, 256),
         ("k_dct8<8, 1, true, false, 4, 0>", 128, 64)]),
    ([64, 64, 37], [("k_dct8<6, 0, true, false, 16, 0>", 148, 64), ("k_dct8<6, 0, false, false, 16, 0>", 148, 64),
         ("k_trigr<32, 16, 64>", 256, 64), ("k_dct8<6, 1, false, false, 16, 0>", 148, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 148, 64)]),
    ([64, 64, 48], [("k_dct8<6, 0, true, false, 16, 0>", 192, 64), ("k_dct8<6, 0, false, false, 16, 0>", 192, 64),
         ("k_trigr<32, 16, 64>", 256, 48), ("k_dct8<6, 1, false, false, 16, 0>", 192, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 192, 64)]),
    ([16, 16, 1024], [("k_plane8<4, 0, false>", 1024, 16), ("k_trir<10, 16, 4>", 64, 256),
         ("k_plane8<4, 1, false>", 1024, 16)]),
    ([64, 64, 64], [("k_dct8<6, 0, true, false, 16, 0>", 256, 64), ("k_dct8<6, 0, false, false, 16, 0>", 256, 64),
         ("k_trir<6, 16, 16>", 256, 64), ("k_dct8<6, 1, false, false, 16, 0>", 256, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 256, 64)]),
    ([500, 500, 2], [("k_dctm<500, 0, true, false, 1>", 500, 50), ("k_dctm<500, 0, false, false, 1>", 500, 50),
         ("k_dctg<2, false, false>", 15625, 512), ("k_dctm<500, 1, false, false, 1>", 500, 50),
         ("k_dctm<500, 1, true, false, 1>", 500, 50)]),
    ([509, 509, 2], [("k_dctb8<10, 0, true, false, 2>", 509, 128), ("k_dctb8<10, 0, false, false, 2>", 509, 128),
         ("k_dctg<2, false, false>", 16193, 512), ("k_dctb8<10, 1, false, false, 2>", 509, 128),
         ("k_dctb8<10, 1, true, false, 2>", 509, 128)]),
    ([64, 64, 128], [("k_dct8<6, 0, true, false, 16, 0>", 512, 64), ("k_dct8<6, 0, false, false, 16, 0>", 512, 64),
         ("k_trir<7, 16, 16>", 256, 128), ("k_dct8<6, 1, false, false, 16, 0>", 512, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 512, 64)]),
    ([512, 512, 2], [("k_dct8<9, 0, true, false, 2, 0>", 512, 64), ("k_dct8<9, 0, false, false, 16, 0>", 64, 512),
         ("k_dct<2, false, false>", 16384, 256), ("k_dct8<9, 1, false, false, 16, 0>", 64, 512),
         ("k_dct8<9, 1, true, false, 2, 0>", 512, 64)]),
    ([128, 128, 37], [("k_dct8<7, 0, true, false, 8, 0>", 592, 64), ("k_dct8<7, 0, false, false, 16, 0>", 296, 128),
         ("k_trigr<16, 64, 8>", 256, 256), ("k_dct8<7, 1, false, false, 16, 0>", 296, 128),
         ("k_dct8<7, 1, true, false, 8, 0>", 592, 64)]),
    ([128, 128, 48], [("k_dct8<7, 0, true, false, 8, 0>", 768, 64), ("k_dct8<7, 0, false, false, 16, 0>", 384, 128),
         ("k_trigr<16, 64, 8>", 256, 192), ("k_dct8<7, 1, false, false, 16, 0>", 384, 128),
         ("k_dct8<7, 1, true, false, 8, 0>", 768, 64)]),
    ([96, 96, 101], [("k_dctg<0, true, false>", 606, 512), ("k_dctg<0, false, false>", 606, 512),
         ("k_trigr<16, 32, 32>", 288, 224), ("k_dctg<1, false, false>", 606, 512),
         ("k_dctg<1, true, false>", 606, 512)]),
    ([96, 96, 113], [("k_dctg<0, true, false>", 678, 512), ("k_dctg<0, false, false>", 678, 512),
         ("k_trigr<16, 32, 32>", 288, 256), ("k_dctg<1, false, false>", 678, 512),
         ("k_dctg<1, true, false>", 678, 512)]),
    ([32, 32, 1024], [("k_plane8<5, 0, false>", 1024, 64), ("k_trir<10, 16, 4>", 256, 256),
         ("k_plane8<5, 1, false>", 1024, 64)]),
    ([64, 64, 256], [("k_dct8<6, 0, true, false, 16, 0>", 1024, 64), ("k_dct8<6, 0, false, false, 16, 0>", 1024, 64),
         ("k_trir<8, 16, 16>", 256, 256), ("k_dct8<6, 1, false, false, 16, 0>", 1024, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 1024, 64)]),
    ([128, 128, 64], [("k_dct8<7, 0, true, false, 8, 0>", 1024, 64), ("k_dct8<7, 0, false, false, 16, 0>", 512, 128),
         ("k_trir<6, 32, 64>", 256, 128), ("k_dct8<7, 1, false, false, 16, 0>", 512, 128),
         ("k_dct8<7, 1, true, false, 8, 0>", 1024, 64)]),
    ([96, 96, 135], [("k_dctg<0, true, false>", 810, 512), ("k_dctg<0, false, false>", 810, 512),
         ("k_trigr<32, 32, 32>", 288, 160), ("k_dctg<1, false, false>", 810, 512),
         ("k_dctg<1, true, false>", 810, 512)]),
    ([128, 128, 101], [("k_dct8<7, 0, true, false, 8, 0>", 1616, 64), ("k_dct8<7, 0, false, false, 16, 0>", 808, 128),
         ("k_trigr<16, 64, 8>", 256, 448), ("k_dct8<7, 1, false, false, 16, 0>", 808, 128),
         ("k_dct8<7, 1, true, false, 8, 0>", 1616, 64)]),
    ([128, 128, 113], [("k_dct8<7, 0, true, false, 8, 0>", 1808, 64), ("k_dct8<7, 0, false, false, 16, 0>", 904, 128),
         ("k_trigr<16, 64, 8>", 256, 512), ("k_dct8<7, 1, false, false, 16, 0>", 904, 128),
         ("k_dct8<7, 1, true, false, 8, 0>", 1808, 64)]),
    ([1000, 1000, 2], [("k_dctm<1000, 0, true, false, 1>", 1000, 50), ("k_dctm<1000, 0, false, false, 1>", 1000, 50),
         ("k_dctg<2, false, false>", 62500, 512), ("k_dctm<1000, 1, false, false, 1>", 1000, 50),
         ("k_dctm<1000, 1, true, false, 1>", 1000, 50)]),
    ([1009, 1009, 2], [("k_dctb8<11, 0, true, false, 4>", 505, 512), ("k_dctb8<11, 0, false, false, 4>", 505, 512),
         ("k_dctg<2, false, false>", 63631, 512), ("k_dctb8<11, 1, false, false, 4>", 505, 512),
         ("k_dctb8<11, 1, true, false, 4>", 505, 512)]),
    ([64, 64, 512], [("k_dct8<6, 0, true, false, 16, 0>", 2048, 64), ("k_dct8<6, 0, false, false, 16, 0>", 2048, 64),
         ("k_trir<9, 16, 16>", 256, 512), ("k_dct8<6, 1, false, false, 16, 0>", 2048, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 2048, 64)]),
    ([128, 128, 128], [("k_dct8<7, 0, true, false, 16, 0>", 1024, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 1024, 128), ("k_trir<7, 32, 64>", 256, 256),
         ("k_dct8<7, 1, false, false, 16, 0>", 1024, 128), ("k_dct8<7, 1, true, false, 16, 0>", 1024, 128)]),
    ([1024, 1024, 2], [("k_dct8<10, 0, true, false, 2, 0>", 1024, 128),
         ("k_dct8<10, 0, false, false, 16, 0>", 128, 1024), ("k_dct<2, false, false>", 65536, 256),
         ("k_dct8<10, 1, false, false, 16, 0>", 128, 1024), ("k_dct8<10, 1, true, false, 2, 0>", 1024, 128)]),
    ([128, 128, 135], [("k_dct8<7, 0, true, false, 16, 0>", 1080, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 1080, 128), ("k_trigr<32, 64, 8>", 256, 320),
         ("k_dct8<7, 1, false, false, 16, 0>", 1080, 128), ("k_dct8<7, 1, true, false, 16, 0>", 1080, 128)]),
    ([251, 251, 37], [("k_dctb8<9, 0, true, false, 16>", 581, 512), ("k_dctb8<9, 0, false, false, 16>", 581, 512),
         ("k_trigr<16, 64, 8>", 985, 256), ("k_dctb8<9, 1, false, false, 16>", 581, 512),
         ("k_dctb8<9, 1, true, false, 16>", 581, 512)]),
    ([128, 128, 160], [("k_dct8<7, 0, true, false, 16, 0>", 1280, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 1280, 128), ("k_trigr<16, 64, 16>", 256, 640),
         ("k_dct8<7, 1, false, false, 16, 0>", 1280, 128), ("k_dct8<7, 1, true, false, 16, 0>", 1280, 128)]),
    ([500, 500, 11], [("k_dctm<500, 0, true, false, 4>", 688, 200), ("k_dctm<500, 0, false, false, 4>", 688, 200),
         ("k_trigr<16, 64, 8>", 3907, 256), ("k_dctm<500, 1, false, false, 4>", 688, 200),
         ("k_dctm<500, 1, true, false, 4>", 688, 200)]),
    ([509, 509, 11], [("k_dctb8<10, 0, true, false, 8>", 700, 512), ("k_dctb8<10, 0, false, false, 8>", 700, 512),
         ("k_trigr<16, 64, 8>", 4049, 256), ("k_dctb8<10, 1, false, false, 8>", 700, 512),
         ("k_dctb8<10, 1, true, false, 8>", 700, 512)]),
    ([96, 96, 400], [("k_dctg<0, true, false>", 2400, 512), ("k_dctg<0, false, false>", 2400, 512),
         ("k_trigr<16, 32, 32>", 288, 800), ("k_dctg<1, false, false>", 2400, 512),
         ("k_dctg<1, true, false>", 2400, 512)]),
    ([128, 128, 241], [("k_dct8<7, 0, true, false, 16, 0>", 1928, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 1928, 128), ("k_trigr<16, 64, 16>", 256, 1024),
         ("k_dct8<7, 1, false, false, 16, 0>", 1928, 128), ("k_dct8<7, 1, true, false, 16, 0>", 1928, 128)]),
    ([128, 128, 251], [("k_dct8<7, 0, true, false, 16, 0>", 2008, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 2008, 128), ("k_trigr<16, 64, 16>", 256, 1024),
         ("k_dct8<7, 1, false, false, 16, 0>", 2008, 128), ("k_dct8<7, 1, true, false, 16, 0>", 2008, 128)]),
    ([64, 64, 1009], [("k_dct8<6, 0, true, false, 16, 0>", 4036, 64), ("k_dct8<6, 0, false, false, 16, 0>", 4036, 64),
         ("k_trigr<32, 16, 64>", 256, 1024), ("k_dct8<6, 1, false, false, 16, 0>", 4036, 64),
         ("k_dct8<6, 1, true, false, 16, 0>", 4036, 64)]),
    ([64, 64, 1024], [("k_plane8<6, 0, false>", 1024, 256), ("k_trir<10, 16, 16>", 256, 1024),
         ("k_plane8<6, 1, false>", 1024, 256)]),
    ([128, 128, 256], [("k_dct8<7, 0, true, false, 16, 0>", 2048, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 2048, 128), ("k_trir<8, 32, 64>", 256, 512),
         ("k_dct8<7, 1, false, false, 16, 0>", 2048, 128), ("k_dct8<7, 1, true, false, 16, 0>", 2048, 128)]),
    ([256, 256, 64], [("k_dct8<8, 0, true, false, 16, 0>", 1024, 256),
         ("k_dct8<8, 0, false, false, 16, 0>", 1024, 256), ("k_trir<6, 32, 64>", 1024, 128),
         ("k_dct8<8, 1, false, false, 16, 0>", 1024, 256), ("k_dct8<8, 1, true, false, 16, 0>", 1024, 256)]),
    ([96, 96, 500], [("k_dctg<0, true, false>", 3000, 512), ("k_dctg<0, false, false>", 3000, 512),
         ("k_trigr<32, 32, 32>", 288, 800), ("k_dctg<1, false, false>", 3000, 512),
         ("k_dctg<1, true, false>", 3000, 512)]),
    ([128, 128, 300], [("k_dct8<7, 0, true, false, 16, 0>", 2400, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 2400, 128), ("k_trigr<32, 64, 16>", 256, 960),
         ("k_dct8<7, 1, false, false, 16, 0>", 2400, 128), ("k_dct8<7, 1, true, false, 16, 0>", 2400, 128)]),
    ([128, 128, 400], [("k_dct8<7, 0, true, false, 16, 0>", 3200, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 3200, 128), ("k_trigr<32, 64, 16>", 256, 1024),
         ("k_dct8<7, 1, false, false, 16, 0>", 3200, 128), ("k_dct8<7, 1, true, false, 16, 0>", 3200, 128)]),
    ([1000, 1000, 8], [("k_dctm<1000, 0, true, false, 4>", 1000, 200),
         ("k_dctm<1000, 0, false, false, 4>", 1000, 200), ("k_trigr<16, 64, 8>", 15625, 128),
         ("k_dctm<1000, 1, false, false, 4>", 1000, 200), ("k_dctm<1000, 1, true, false, 4>", 1000, 200)]),
    ([128, 128, 500], [("k_dct8<7, 0, true, false, 16, 0>", 4000, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 4000, 128), ("k_trigr<32, 64, 16>", 256, 1024),
         ("k_dct8<7, 1, false, false, 16, 0>", 4000, 128), ("k_dct8<7, 1, true, false, 16, 0>", 4000, 128)]),
    ([2039, 2039, 2], [("k_dctb8<12, 0, true, false, 2>", 2039, 512), ("k_dctb8<12, 0, false, false, 2>", 2039, 512),
         ("k_dctg<2, false, false>", 259846, 512), ("k_dctb8<12, 1, false, false, 2>", 2039, 512),
         ("k_dctb8<12, 1, true, false, 2>", 2039, 512)]),
    ([128, 128, 512], [("k_dct8<7, 0, true, false, 16, 0>", 4096, 128),
         ("k_dct8<7, 0, false, false, 16, 0>", 4096, 128), ("k_trir<9, 16, 32>", 512, 1024),
         ("k_dct8<7, 1, false, false, 16, 0>", 4096, 128), ("k_dct8<7, 1, true, false, 16, 0>", 4096, 128)]),
    ([512, 512, 32], [("k_dct8<9, 0, true, false, 16, 0>", 1024, 512),
         ("k_dct8<9, 0, false, false, 16, 0>", 1024, 512), ("k_dct8<5, 2, false, false, 16, 0>", 16384, 32),
         ("k_dct8<9, 1, false, false, 16, 0>", 1024, 512), ("k_dct8<9, 1, true, false, 16, 0>", 1024, 512)]),
    ([1024, 1024, 8], [("k_dct8<10, 0, true, false, 8, 0>", 1024, 512),
         ("k_dct8<10, 0, false, false, 16, 0>", 512, 1024), ("k_dct8<3, 2, false, false, 16, 0>", 65536, 8),
         ("k_dct8<10, 1, false, false, 16, 0>", 512, 1024), ("k_dct8<10, 1, true, false, 8, 0>", 1024, 512)]),
    ([2048, 2048, 2], [("k_dct8<11, 0, true, false, 4, 0>", 1024, 512),
         ("k_dct8<11, 0, false, false, 8, 0>", 512, 1024), ("k_dct<2, false, false>", 262144, 256),
         ("k_dct8<11, 1, false, false, 8, 0>", 512, 1024), ("k_dct8<11, 1, true, false, 4, 0>", 1024, 512)]),
    ([128, 128, 1024], [("k_plane8<7, 0, false>", None, 1024), ("k_trir<10, 32, 32>", 512, 1024),
         ("k_plane8<7, 1, false>", None, 1024)]),
    ([8, 8, 8, 8], [("k_dct8<3, 0, true, false, 16, 0>", 32, 8), ("k_dct8<3, 0, false, false, 16, 0>", 64, 8),
         ("k_dct8<3, 0, false, false, 16, 0>", 32, 8), ("k_dct8<3, 2, false, false, 16, 0>", 32, 8),
         ("k_dct8<3, 1, false, false, 16, 0>", 32, 8), ("k_dct8<3, 1, false, false, 16, 0>", 64, 8),
         ("k_dct8<3, 1, true, false, 16, 0>", 32, 8)]),
    ([12, 12, 12, 16], [("k_dctg<0, true, false>", 576, 512), ("k_dctg<0, false, false>", 576, 512),
         ("k_dctg<0, false, false>", 576, 512), ("k_trigr<32, 4, 64>", 432, 8), ("k_dctg<1, false, false>", 576, 512),
         ("k_dctg<1, false, false>", 576, 512), ("k_dctg<1, true, false>", 576, 512)]),
    ([12, 12, 12, 32], [("k_dctg<0, true, false>", 576, 512), ("k_dctg<0, false, false>", 576, 512),
         ("k_dctg<0, false, false>", 576, 512), ("k_trigr<32, 4, 64>", 432, 8), ("k_dctg<1, false, false>", 576, 512),
         ("k_dctg<1, false, false>", 576, 512), ("k_dctg<1, true, false>", 576, 512)]),
    ([12, 12, 12, 64], [("k_dctg<0, true, false>", 576, 512), ("k_dctg<0, false, false>", 576, 512),
         ("k_dctg<0, false, false>", 576, 512), ("k_trigr<32, 4, 64>", 432, 16),
         ("k_dctg<1, false, false>", 576, 512), ("k_dctg<1, false, false>", 576, 512),
         ("k_dctg<1, true, false>", 576, 512)]),
    ([16, 16, 16, 64], [("k_plane8<4, 0, false>", 1024, 16), ("k_dct8<4, 0, false, false, 16, 0>", 1024, 16),
         ("k_trir<6, 16, 16>", 256, 64), ("k_dct8<4, 1, false, false, 16, 0>", 1024, 16),
         ("k_plane8<4, 1, false>", 1024, 16)]),
    ([32, 32, 32, 64], [("k_plane8<5, 0, false>", 2048, 64), ("k_dct8<5, 0, false, false, 16, 0>", 4096, 32),
         ("k_trir<6, 32, 64>", 512, 128), ("k_dct8<5, 1, false, false, 16, 0>", 4096, 32),
         ("k_plane8<5, 1, false>", 2048, 64)]),
]

# the same solve under the other block order and with unit weights (ORDER_PY, weighted=False): (mesh, order, weighted)
VARIANTS = [([64, 64, 64], "py", True), ([4096, 64], "cpp", False)]

_EXPECT = {tuple(m): log for m, log in DISPATCH}


def _sigmas(m):
    return SIGMAS if int(np.prod(m)) <= (1 << 23) else SIGMAS_BIG


_PARAMS = [(tuple(m), "cpp", True, s) for m, _ in DISPATCH for s in _sigmas(m)]
_PARAMS += [(tuple(m), o, w, s) for m, o, w in VARIANTS for s in _sigmas(m)]


def _id(v):
    if isinstance(v, (tuple, list)):
        return "x".join(str(x) for x in v)
    return str(v)


@functools.lru_cache(maxsize=1)
def _case(m, order, weighted):
    """Everything one mesh's cases share, built once (the parameters run mesh-major): the problem on the GPU, b, and
    the forward transforms and symbols of the long-double reference and of its float64 evaluation."""
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP if order == "cpp" else mv.ORDER_PY, weighted=weighted)
    assert P.spectral_ok()
    ref = {}
    for name, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[name] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, order, weighted, dtype))
    return P, b, ref


def check_log(log, expect):
    """the launch log of one solve against the table: names and blocks, grids where the table gives one"""
    got = [(name, grid[0], block[0]) for name, grid, block in log]
    assert [g[0] for g in got] == [e[0] for e in expect], got
    for (name, grid, block), (_, egrid, eblock) in zip(got, expect):
        assert block == eblock and (egrid is None or grid == egrid), (name, grid, block, egrid, eblock)
    assert all(grid[1:] == (1, 1) and block[1:] == (1, 1) for _, grid, block in log)


@pytest.mark.parametrize("m,order,weighted,sigma", _PARAMS, ids=_id)
def test_dispatch_and_forward_error(m, order, weighted, sigma):
    P, b, ref = _case(m, order, weighted)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    check_log(log, _EXPECT[m])
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    assert scale >= abs(float(b.mean())) * (1.0 - 1e-12)   # the mean of b passes through unchanged
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    tag = "" if (order, weighted) == ("cpp", True) else f" {order} weighted={weighted}"
    print(f"dispatch {_id(m)}{tag} sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
    log_parity(f"dispatch {_id(m)}{tag} sigma={sigma:g}", e64=e64, err=err, kernels=" | ".join(n for n, _, _ in log))
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


# --------------------------------------------------------------------------------------------------------------------
# First passes that run only inside the ADMM loop: b formed on load (plain, and from the folded s of the fused 3-D
# kernel: the same instantiation, told by its control block) and the PCG-fused d = 0 passes. solve_spectral reaches none.
ADMM_LAM, ADMM_RHO0, ADMM_ITERS = 0.8, 0.004, 4   # rho0 = lam / 200: adapt_step doubles rho in the first iterations

# (mesh, the first pass the loop must launch); W = I, against the C oracle's loop with scipy.fft's exact solve
FIRST_PASS = [
    ([4], "k_dct<2, true, true>"), ([8], "k_dct8<3, 2, true, true, 16, 0>"), ([16], "k_dct8<4, 2, true, true, 16, 0>"),
    ([32], "k_dct8<5, 2, true, true, 16, 0>"), ([64], "k_dct8<6, 2, true, true, 16, 0>"),
    ([128], "k_dct8<7, 2, true, true, 8, 0>"), ([256], "k_dct8<8, 2, true, true, 4, 0>"),
    ([512], "k_dct8<9, 2, true, true, 2, 0>"), ([1024], "k_dct8<10, 2, true, true, 2, 0>"),
    ([2048], "k_dct8<11, 2, true, true, 2, 0>"), ([4096], "k_dct8<12, 2, true, true, 2, 0>"),
    ([100], "k_dctg<2, true, true>"), ([37], "k_dctb8<7, 2, true, true, 16>"),
    ([4, 4], "k_dct<0, true, true>"), ([8, 8], "k_dct8<3, 0, true, true, 16, 0>"),
    ([16, 16], "k_dct8<4, 0, true, true, 16, 0>"), ([32, 32], "k_dct8<5, 0, true, true, 16, 0>"),
    ([64, 64], "k_dct8<6, 0, true, true, 16, 0>"), ([128, 128], "k_dct8<7, 0, true, true, 8, 0>"),
    ([256, 256], "k_dct8<8, 0, true, true, 4, 0>"), ([512, 512], "k_dct8<9, 0, true, true, 2, 0>"),
    ([1024, 64], "k_dct8<10, 0, true, true, 2, 0>"), ([2048, 8], "k_dct8<11, 0, true, true, 2, 0>"),
    ([4096, 4], "k_dct8<12, 0, true, true, 2, 0>"), ([12, 12], "k_dctg<0, true, true>"),
    ([500, 8], "k_dctm<500, 0, true, true, 1>"), ([500, 4096], "k_dctm<500, 0, true, true, 4>"),
    ([31, 31], "k_dctb8<6, 0, true, true, 16>"), ([37, 37], "k_dctb8<7, 0, true, true, 16>"),
    ([67, 8], "k_dctb8<8, 0, true, true, 16>"), ([251, 8], "k_dctb8<9, 0, true, true, 2>"),
    ([1009, 8], "k_dctb8<11, 0, true, true, 4>"), ([2039, 4], "k_dctb8<12, 0, true, true, 2>"),
    ([4093, 2], "k_dctb8<13, 0, true, true, 2>"), ([2048, 4096], "k_dct8<11, 0, true, true, 4, 0>"),
    ([128, 128, 128], "k_dct8<7, 0, true, true, 16, 0>"), ([256, 256, 64], "k_dct8<8, 0, true, true, 16, 0>"),
    ([512, 512, 32], "k_dct8<9, 0, true, true, 16, 0>"), ([1024, 1024, 8], "k_dct8<10, 0, true, true, 8, 0>"),
    ([251, 251, 37], "k_dctb8<9, 0, true, true, 16>"), ([16, 16, 1024], "k_plane8<4, 0, true>"),
    ([32, 32, 1024], "k_plane8<5, 0, true>"), ([64, 64, 1024], "k_plane8<6, 0, true>"),
    ([11, 11, 11, 2], "k_dctb8<5, 0, true, true, 32>"),
]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize("m,kernel", FIRST_PASS, ids=_id)
def test_first_pass_in_admm_loop(m, kernel):
    """Variant B, W = I, 4 fixed iterations from a rho0 that adapt_step changes (so the first pass runs both from
    g_alpha / g_u and, on the fused 3-D path, from the folded s with and without the g_u correction) against the C
    oracle's loop with scipy.fft's exact solve: rho exact, theta and u to 1e-10 (test_bluestein_admm_vs_c_oracle)."""
    from multivartv_amd.synth import towers
    from oracle import c_oracle
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(y.size, y.mean())
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert P.spectral_ok()
        P.state_set(th0, None, ADMM_RHO0)
        with launch_log() as log:
            st = P.run(ADMM_LAM, fixed_iters=ADMM_ITERS)
        tg, ug, rg = P.state_get(want_u=True)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL and st["iters"] == ADMM_ITERS
    names = [n for n, _, _ in log]
    assert names.count(kernel) >= ADMM_ITERS, sorted(set(names))
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp_spectral(m, y, ADMM_LAM, th, u, ADMM_RHO0, deltas, fixed_iters=ADMM_ITERS,
                                      workers=WORKERS)
    assert ref["rho"] != ADMM_RHO0          # adapt_step changed rho: the loop took a first pass after a rho change
    assert rg == ref["rho"]
    et, eu = _rel(tg, th), float(np.max(np.abs(ug - u)) / max(1.0, np.max(np.abs(u))))
    log_parity(f"first pass {_id(tuple(m))} {kernel}", theta=et, u=eu)
    assert et <= 1e-10
    assert eu <= 1e-10


# (mesh, the PCG-fused first and last pass of every preconditioner solve); W = a CV-fold mask
PCG_FUSED = [
    ([64, 64], "k_dct8<6, 0, true, false, 16, 1>", "k_dct8<6, 1, true, false, 16, 2>"),
    ([128, 128], "k_dct8<7, 0, true, false, 8, 1>", "k_dct8<7, 1, true, false, 8, 2>"),
    ([256, 256], "k_dct8<8, 0, true, false, 4, 1>", "k_dct8<8, 1, true, false, 4, 2>"),
    ([512, 512], "k_dct8<9, 0, true, false, 2, 1>", "k_dct8<9, 1, true, false, 2, 2>"),
    ([1024, 64], "k_dct8<10, 0, true, false, 2, 1>", "k_dct8<10, 1, true, false, 2, 2>"),
    ([2048, 8], "k_dct8<11, 0, true, false, 2, 1>", "k_dct8<11, 1, true, false, 2, 2>"),
    ([4096, 4], "k_dct8<12, 0, true, false, 2, 1>", "k_dct8<12, 1, true, false, 2, 2>"),
    ([128, 128, 128], "k_dct8<7, 0, true, false, 16, 1>", "k_dct8<7, 1, true, false, 16, 2>"),
]


@pytest.mark.parametrize("m,first,last", PCG_FUSED, ids=_id)
def test_pcg_fused_passes(m, first, last):
    """W != I (one CV fold held out), PCG with the cosine-transform preconditioner: the x / r update rides on the
    preconditioner's first d = 0 pass, the scaling and r.z on its last (k_dct8<.., 1> / <.., 2>). Against the C oracle's
    Jacobi-PCG loop at the same tolerance: rho exact, theta to 1e-9 (test_spectrally_preconditioned_pcg)."""
    from multivartv_amd.synth import towers
    from oracle import c_oracle
    y = towers(m, seed=len(m))
    W = (np.random.default_rng(len(m)).permutation(y.size) % 5 != 0).astype(float)
    oty = W * y
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(W.size, oty.sum() / W.sum())
    lam, rho0, iters = 0.5, 0.1, 3
    with mv.Problem(m, oty, wdiag=W, deltas=deltas, order=mv.ORDER_CPP) as P:
        with launch_log() as log:
            tg, ug, rg, st = P.admm(lam, th0, u=np.zeros(P.E), rho=rho0, fixed_iters=iters, pcg_rtol=1e-13,
                                    theta_solver=mv.SOLVER_PCG_SPECTRAL)
    assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["pcg_unconverged"] == 0
    names = [n for n, _, _ in log]
    assert not names[0].startswith("#"), names[0]
    assert names.count(first) >= iters and names.count(first) == names.count(last), sorted(set(names))
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp(m, oty, lam, th, u, rho0, deltas, W=W, fixed_iters=iters, pcg_rtol=1e-13)
    assert rg == ref["rho"]
    et = _rel(tg, th)
    log_parity(f"pcg fused {_id(tuple(m))} {first}", theta=et, pcg_iters=int(st["pcg_iters"]))
    assert et <= 1e-9
