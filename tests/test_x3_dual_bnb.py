"""When the fp32-emulating dual launch may do batch norm's backward inside its dA blocks (csrc/x3_layout.h: dual_bnb_eligible;
csrc/gemm_bf16.hip: EPI_DACT_BN), on the CPU, through tools/x3_dual_bnb_check.cpp, which calls the function the launcher calls.

The rule under test -- eligible exactly when
  * the pass is not stacked,
  * the apply kernel's chunk of rows divides the 128-row tile of the contraction (a chunk never straddles two tiles),
  * dA is the problem with the longer K (frames <= K of dA), so each of its tiles has a block of its own, and
  * the per-tile partial sums fit the slots the apply kernel sums itself (no more row tiles than `max_tiles`)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 128


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


def _chunk_rows(T, rows):
    """rows per block of the column-tiled kernels (csrc/kernels.hip: row_splits, at most 256 blocks along T)"""
    rs = min(max(-(-T // rows), 1), 256)
    return -(-T // rs)


def test_eligible_exactly_when_chunks_tile_the_tile_and_dA_is_the_long_side(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "x3_dual_bnb_check")
    subprocess.run([cc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tfkaldi_amd", "csrc"),
                    os.path.join(ROOT, "tools", "x3_dual_bnb_check.cpp"), "-o", exe], check=True)
    cases = []
    for T in range(1, 4097):
        for rows in (8, 16, 24, 29, 32, 48, 64):
            for k_da, stacked, max_tiles in ((2048, 0, 32), (2048, 1, 32), (1000, 0, 32), (4096, 0, 8), (T, 0, 32), (T - 1, 0, 32)):
                cases.append((T, _chunk_rows(T, rows), k_da, stacked, max_tiles))
    # chunk sizes given directly, whatever frame count would produce them
    cases += [(1024, c, 2048, 0, 32) for c in range(1, 130)] + [(1024, 0, 2048, 0, 32), (0, 32, 2048, 0, 32), (1024, 32, 2048, 0, 7),
                                                                  (1024, 32, 2048, 0, 8)]
    r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
    got = [int(v) for v in r.stdout.split()]
    assert len(got) == len(cases)
    yes = 0
    for (T, chunk, k_da, stacked, max_tiles), g in zip(cases, got):
        want = (not stacked and T >= 1 and chunk >= 1 and TILE % chunk == 0 and T <= k_da and -(-T // TILE) <= max_tiles)
        assert bool(g) == want, (T, chunk, k_da, stacked, max_tiles, g)
        yes += g
    assert 0 < yes < len(cases)
    # the flagship shape and its neighbours: 1024 frames in chunks of 32 rows, K = 2048
    at = {c: g for c, g in zip(cases, got)}
    assert at[(1024, 32, 2048, 0, 32)] == 1 and at[(1024, 32, 2048, 1, 32)] == 0 and at[(1024, 32, 1000, 0, 32)] == 0
    assert at[(200, _chunk_rows(200, 32), 2048, 0, 32)] == 0  # 7 chunks of 29 rows: a chunk would straddle the two tiles
    assert at[(1000, 32, 2048, 0, 32)] == 1                   # a partial last chunk is fine
