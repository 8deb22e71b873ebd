"""The host side of streaming CTC decoding, on the CPU.
1. processing.feature_reader.StreamSplicer: the rows of all pushes plus the flush equal splice(normalised(all frames), c) bit for
   bit for any chunking -- for an utterance shorter than 2c + 1, where splice returns None, the zero-padded splice written out by
   hand here -- and no push returns a row before its right context exists.
2. The limits, push / result checks and the layout of a stream's allocation (csrc/ctc_tables.h) through
   tools/ctc_stream_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  Every expected message is a literal.
"""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tfkaldi_amd import _lib
from tfkaldi_amd.processing.feature_reader import StreamSplicer, Unspliced, splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 3


# ---- 1. StreamSplicer ----

def _padded_splice(x, c):
    """the zero-padded splice, written out: block j of row t is frame t + j - c, zero outside the utterance"""
    n, d = x.shape
    out = np.zeros((n, d * (2 * c + 1)), dtype=np.float32)
    for t in range(n):
        for j in range(2 * c + 1):
            s = t + j - c
            if 0 <= s < n:
                out[t, j * d:(j + 1) * d] = x[s]
    return out


def _expected(frames, c, cmvn):
    x = Unspliced(frames, c, cmvn=cmvn).normalised()
    want = splice(np.asarray(x), c)
    if want is None:
        assert frames.shape[0] < 2 * c + 1
        return _padded_splice(np.asarray(x, dtype=np.float32), c)
    assert np.array_equal(want.view(np.uint32), _padded_splice(np.asarray(x), c).view(np.uint32))
    return want


def _chunkings(N, rng):
    yield "whole", [N]
    yield "ones", [1] * N
    if N >= 1:
        yield "[1, N-1]", [1, N - 1]
        yield "[N-1, 1]", [N - 1, 1]
    for k in range(3):
        cuts = sorted(rng.integers(0, N + 1, size=3).tolist())
        sizes = np.diff([0] + cuts + [N]).tolist()
        mixed = []
        for s in sizes:  # empty chunks in between
            mixed += [s, 0]
        yield "random %d" % k, [0] + mixed


@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("c", [0, 1, 5])
def test_stream_splicer_equals_splice(c, with_cmvn):
    rng = np.random.default_rng(100 * c + with_cmvn)
    cmvn = None
    if with_cmvn:
        cmvn = np.stack([rng.normal(size=D), rng.uniform(0.5, 2.0, size=D)]).astype(np.float32)
    sp = StreamSplicer(D, c, cmvn=cmvn)
    for N in sorted({0, 1, c, 2 * c, 2 * c + 1, 40}):
        frames = rng.normal(size=(N, D)).astype(np.float32)
        want = _expected(frames, c, cmvn)
        assert want.shape == (N, D * (2 * c + 1))
        for name, sizes in _chunkings(N, rng):
            assert sum(sizes) == N
            got, at = [], 0
            for n in sizes:
                rows = sp.push(frames[at:at + n])
                at += n
                got.append(rows)
                done = sum(r.shape[0] for r in got)
                assert rows.dtype == np.float32 and rows.shape[1] == D * (2 * c + 1)
                assert done == max(at - c, 0), (name, N, at, done)  # exactly the rows whose right context has arrived
            got.append(sp.flush())  # (also leaves the object ready for the next utterance: every case reuses it)
            got = np.concatenate(got)
            assert got.shape == want.shape, (name, N)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, N, c, with_cmvn)
        print("StreamSplicer c=%d cmvn=%d N=%d: %d chunkings equal splice()" % (c, with_cmvn, N, 4 + 3 if N else 1 + 3))


def test_stream_splicer_second_utterance_and_cmvn_change():
    rng = np.random.default_rng(7)
    a, b = (rng.normal(size=(n, D)).astype(np.float32) for n in (9, 4))
    table = np.stack([rng.normal(size=D), rng.uniform(0.5, 2.0, size=D)]).astype(np.float32)
    sp = StreamSplicer(D, 2)
    first = np.concatenate([sp.push(a[:5]), sp.push(a[5:]), sp.flush()])
    sp.set_cmvn(table)
    second = np.concatenate([sp.push(b), sp.flush()])
    assert np.array_equal(first, _expected(a, 2, None))
    assert np.array_equal(second, _expected(b, 2, table))  # 4 < 2c + 1: the padded form
    with pytest.raises(ValueError):
        StreamSplicer(0, 1)
    with pytest.raises(ValueError):
        sp.push(np.zeros((2, D + 1), dtype=np.float32))


# ---- 2. limits and layout through the stand-alone tool ----

def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ctc_stream") / "ctc_stream_check")
    subprocess.run([cc, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "tfkaldi_amd", "csrc"), os.path.join(ROOT, "tools", "ctc_stream_check.cpp"), "-o", exe],
                   check=True)

    def run(commands):
        # (the leak pass needs to stop the process's threads, which some sandboxes forbid; the memory and UB checks stay on)
        r = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.split("\n")
        assert len(lines) == len(commands) + 1 and lines[-1] == ""
        return [l.split(";") for l in lines[:-1]]
    return run


def _arr(v):
    return "NULL" if v is None else " ".join(str(x) for x in v)


def test_stream_limits(tool):
    def lim(O, lanes, W, mf, K):
        return "limits;%d;%d;%d;%d;%d" % (O, lanes, W, mf, K)
    cases = [
        (lim(64, 1, 128, 524286, 0), ""), (lim(2, 1024, 1, 1, 0), ""), (lim(65536, 3, 16, 64, 63), ""), (lim(300, 3, 16, 64, 5), ""),
        (lim(9, 0, 8, 64, 0), "stream: lanes 0 outside [1, 1024]"),
        (lim(9, 1025, 8, 64, 0), "stream: lanes 1025 outside [1, 1024]"),
        (lim(9, 3, 0, 64, 0), "stream: beam_width 0 outside [1, 128]"),
        (lim(9, 3, 129, 64, 0), "stream: beam_width 129 outside [1, 128]"),
        (lim(9, 3, 8, 0, 0), "stream: max_frames 0 outside [1, 524286]"),
        (lim(9, 3, 8, 524287, 0), "stream: max_frames 524287 outside [1, 524286]"),
        (lim(9, 3, 8, 64, -1), "stream: label_topk -1 outside [0, 63]"),
        (lim(9, 3, 8, 64, 64), "stream: label_topk 64 outside [0, 63]"),
        (lim(1, 3, 8, 64, 0), "stream: output_dim 1 outside [2, 64] (63 labels + blank, more with label_topk)"),
        (lim(65, 3, 8, 64, 0), "stream: output_dim 65 outside [2, 64] (63 labels + blank, more with label_topk)"),
        (lim(1, 3, 8, 64, 5), "stream: output_dim 1 outside [2, 65536]"),
        (lim(65537, 3, 8, 64, 5), "stream: output_dim 65537 outside [2, 65536]"),
    ]
    for (cmd, message), got in zip(cases, tool([c for c, _ in cases])):
        assert got == (["0", ""] if not message else ["-1", message]), (cmd, got)


def test_stream_push_and_result_checks(tool):
    def push(T, mf, chunk, frames):
        return "push;%d;%d;%s;%s" % (T, mf, _arr(chunk), _arr(frames))
    cases = [
        (push(7, 64, [3, 4, 0], [0, 0, 0]), ""),
        (push(0, 64, [0, 0, 0], [64, 0, 3]), ""),
        (push(4, 64, [0, 4, 0], [64, 60, 0]), ""),  # exactly max_frames
        (push(7, 64, None, [0, 0, 0]), "push: chunk_len is NULL"),
        (push(-1, 64, [0, 0, 0], [0, 0, 0]), "push: T = -1 < 0"),
        (push(7, 64, [3, -1, 5], [0, 0, 0]), "push: lane 1 has a negative chunk length"),
        (push(7, 64, [3, 3, 0], [0, 0, 0]), "push: the chunk lengths sum to 6, expected T = 7"),
        (push(5, 64, [0, 5, 0], [64, 60, 0]), "push: lane 1 would hold 65 frames (max_frames 64)"),
        (push(1, 64, [1, 0, 0], [64, 0, 0]), "push: lane 0 would hold 65 frames (max_frames 64)"),
        (push(2147483647, 524286, [2147483647], [524286]), "push: lane 0 would hold 2148007933 frames (max_frames 524286)"),
        ("result;8;1;0", ""), ("result;8;8;100", ""),
        ("result;8;0;4", "result: top_paths 0 outside [1, beam_width = 8]"),
        ("result;8;9;4", "result: top_paths 9 outside [1, beam_width = 8]"),
        ("result;8;1;-1", "result: hyp_cap -1 < 0"),
    ]
    for (cmd, message), got in zip(cases, tool([c for c, _ in cases])):
        assert got == (["0", ""] if not message else ["-1", message]), (cmd, got)


def test_stream_layout(tool):
    shapes = list(itertools.product((1, 3), (1, 128), (1, 64)))
    lib = _lib.load()
    got = tool(["layout;%d;%d;%d" % s for s in shapes])
    for (lanes, W, mf), line in zip(shapes, got):
        trie, hdr, arr, seg, total, lane_words = (int(v) for v in line[0].split())
        assert lane_words == 2 * mf * W + 64
        # [start, bytes, element size]: the trie's 64-bit words, the headers (8 words per lane, a double at word 4), the beam arrays
        # (11 per lane), the chunk bounds
        regions = [(trie, lanes * lane_words * 8, 8), (hdr, lanes * 8 * 4, 8), (arr, lanes * 11 * W * 4, 4), (seg, (lanes + 1) * 4, 4)]
        for start, size, elem in regions:
            assert start % elem == 0 and size > 0 and start + size <= total, (lanes, W, mf, regions, total)
        for (a, an, _), (b, bn, _) in itertools.combinations(regions, 2):
            assert a + an <= b or b + bn <= a, (lanes, W, mf, regions)
        assert total == sum(size for _, size, _ in regions)  # nothing beyond the regions
        assert total >= 16 * mf * W * lanes
        for l in range(lanes):  # a lane's header, and the double inside it, are 8-byte aligned
            assert (hdr + l * 8 * 4 + 16) % 8 == 0
        for label_topk in (0, 5):  # what the library reports for the shape, pruned or not: the same allocation
            n = ctypes.c_size_t()
            assert lib.tfk_ctc_stream_bytes(9, lanes, W, mf, label_topk, ctypes.byref(n)) == 0, lib.tfk_last_error()
            assert n.value == total
        print("layout lanes=%d W=%d max_frames=%d: %d bytes, %d per lane in the trie" % (lanes, W, mf, total, lane_words * 8))
