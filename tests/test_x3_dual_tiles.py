"""The tile lists of the fp32-emulating dual launch (csrc/x3_layout.h: dual_tiles_per_block, dual_short_blocks,
dual_block_tiles; csrc/gemm_bf16.hip: gemm_bf16x3_dual_kernel) on the CPU, through tools/x3_dual_tiles_check.cpp, which calls the
functions the launcher and the kernel call.  A block of the problem with the shorter K runs a list of consecutive tiles of one
XCD's run of the tile sequence; the rule under test:
  * every tile of the short problem is given to exactly one block, inside the run of the XCD the block shares with the blocks
    of the same index modulo 8, full lists first and at most one shorter list at the end of a run;
  * the ring tiles of a full list differ from a long block's by at most one short tile's length -- unless that many tiles per
    block would leave the grid with fewer blocks than the chip has CUs (256): then the count is the largest one that does not
    (an idle CU costs more than a ramp), and the test checks exactly that;
  * the grid ends with a block that has work."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS, XCDS = 256, 8


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


def _problems():
    """(n_long, nk_long, n_short, nk_short) of the backward pair of a layer [frames, d_in] x [d_in, d_out]"""
    t128 = lambda n: (n + 127) // 128  # noqa: E731
    nk = lambda k: (k + 31) // 32  # noqa: E731
    shapes = [(1024, 2048, 2048), (1024, 2048, 2000), (1024, 2176, 1920), (1000, 2050, 2010), (64, 4096, 4096), (96, 4096, 4096),
              (40, 4096, 4096), (8192, 2048, 2048)]
    shapes += list(itertools.product([64, 100, 512, 1000, 1024, 2048, 3000, 8192, 16384], [440, 1024, 2048, 2176, 4096], [1920, 2000, 2048, 4096]))
    out = []
    for frames, d_in, d_out in shapes:
        n_a, k_a = t128(frames) * t128(d_in), d_out    # dA[frames, d_in] over K = d_out
        n_w, k_w = t128(d_in) * t128(d_out), frames    # dW[d_in, d_out] over K = frames
        if n_a + n_w < CUS:
            continue  # (the dual entry declines such a pair)
        out.append((n_w, nk(k_w), n_a, nk(k_a)) if k_w > k_a else (n_a, nk(k_a), n_w, nk(k_w)))
    # small and odd tile counts, whatever shape would give them
    out += [(300, 7, n, 3) for n in (1, 5, 8, 9, 17, 63, 255, 257)] + [(1, 64, 300, 1), (0, 1, 256, 1), (250, 3, 13, 3)]
    return out


def test_every_tile_once_and_lists_as_equal_as_the_counts_allow(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "x3_dual_tiles_check")
    subprocess.run([cc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tfkaldi_amd", "csrc"),
                    os.path.join(ROOT, "tools", "x3_dual_tiles_check.cpp"), "-o", exe], check=True)
    problems = _problems()
    assert len(problems) > 150
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % p for p in problems), capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")
    at = 0
    lists_seen = 0
    for n_long, nk_long, n_short, nk_short in problems:
        tag, per, blocks = lines[at].split()
        assert tag == "P"
        per, blocks = int(per), int(blocks)
        rows = [tuple(int(v) for v in l.split()[1:]) for l in lines[at + 1:at + 1 + blocks]]
        at += 1 + blocks
        what = (n_long, nk_long, n_short, nk_short, per)
        # ---- tiles per block ----
        assert per >= 1, what
        cap_ok = lambda c: n_long + -(-n_short // c) >= CUS  # noqa: E731
        off = lambda c: abs(c * nk_short - nk_long)  # noqa: E731
        if per > 1:
            assert cap_ok(per), what  # never fewer blocks than CUs for the sake of a list
            assert off(per) < off(per - 1), what  # and never more tiles than bring a list closer to a long block
        # a full list within one short tile's length of a long block, and no count closer to it -- or one more tile per block
        # would leave CUs without a block
        assert (off(per) <= nk_short and off(per + 1) >= off(per)) or not cap_ok(per + 1), what
        # ---- every tile once, inside its XCD's run ----
        q, rem = divmod(n_short, XCDS)
        seen = [0] * n_short
        for g, (seq0, count) in enumerate(rows):
            x, j = g % XCDS, g // XCDS
            start = x * (q + 1) if x < rem else rem * (q + 1) + (x - rem) * q
            cnt = q + (1 if x < rem else 0)
            assert 0 <= count <= per, (what, g)
            if count:
                assert start <= seq0 and seq0 + count <= start + cnt, (what, g)
                assert seq0 == start + j * per, (what, g)  # consecutive lists of a run follow each other
                assert count == per or seq0 + count == start + cnt, (what, g)  # only a run's last list is short
            for s in range(seq0, seq0 + count):
                seen[s] += 1
            lists_seen += count > 1
        assert all(v == 1 for v in seen), what
        assert blocks == 0 or rows[-1][1] > 0, what  # the grid ends with work
        assert sum(1 for _, c in rows if c == 0) < XCDS, what
    assert lists_seen > 1000  # (the grid does exercise lists)
    assert at == len(lines) - 1 and lines[-1] == ""


def test_the_bench_shape_gets_one_block_per_cu(tmp_path):
    """1024 frames, 2048 x 2048: 128 dA tiles of 64 ring tiles + 256 dW tiles of 32 -> 128 + 128 blocks, two dW tiles each;
    8192 stacked rows: 256 dW tiles of 256 ring tiles + 1024 dA tiles of 64 -> four dA tiles per block"""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "x3_dual_tiles_check")
    subprocess.run([cc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tfkaldi_amd", "csrc"),
                    os.path.join(ROOT, "tools", "x3_dual_tiles_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="128 64 256 32\n256 256 1024 64\n", capture_output=True, text=True, check=True)
    heads = [l.split() for l in r.stdout.split("\n") if l.startswith("P")]
    assert heads == [["P", "2", "128"], ["P", "4", "256"]]
