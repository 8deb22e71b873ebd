"""The fp32-emulating dual launch (tfk_gemm_bf16x3_dual: dA = dZ . W^T and G (+)= in^T . dZ of a layer in ONE launch) with
several tiles per block (csrc/gemm_bf16.hip: dma_tile, LIST; csrc/x3_layout.h: dual_tiles_per_block).  A block of the problem with
the shorter K runs a list of tiles, the ring of LDS slots carrying on from one tile into the next; no addition changes place,
so for every shape below

  (a) dA and G lie within x3_error_bound(K) * sum|a b| of the float64 product (tests/test_gpu_f32x3.py: the bound the
      stand-alone contraction is held to, whatever the data), and
  (b) they equal BITWISE the single GEMM_NT / GEMM_TN contraction (tfk_gemm_bf16x3) of the same operands wherever that
      contraction runs unsplit 128x128 blocks over all of K -- it does when its result has at least 200 such tiles
      (gemm_bf16.hip: launch_x3).  Below that the single call splits its K in two or runs another block shape, its additions
      are grouped differently, and (a) alone holds: `_single_is_unsplit_128` says which, and the test prints it.

The dual entry declines pairs with fewer than 256 tiles, so every case keeps at least that many."""
import ctypes
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
p4 = lambda n: (n + 3) & ~3  # noqa: E731


def _single_is_unsplit_128(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128) >= 200


def _planes(lib, x):
    from tfkaldi_amd import x3
    return x3.split(lib, x)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _dual(lib, dz, w, x, dA, G, epi_tn):
    """dA[T, d_in] = dz[T, d_out] . w[d_in, d_out]^T;  G[d_in, d_out] (+)= x[T, d_in]^T . dz"""
    import torch
    from tfkaldi_amd import _lib
    T, d_out = dz[2]
    d_in = w[2][0]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tfk_gemm_bf16x3_dual(st, _ptr(dz[0]), dz[1], _ptr(w[0]), w[1], _ptr(dA), dA.shape[1], T, d_in, d_out,
                                        _ptr(x[0]), x[1], _ptr(dz[0]), dz[1], _ptr(G), G.shape[1], d_in, d_out, T, epi_tn))


def _single(lib, layout, a, b, C, M, N, K, epi):
    import torch
    from tfkaldi_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tfk_gemm_bf16x3(st, layout, _ptr(a[0]), a[1], _ptr(b[0]), b[1], _ptr(C), C.shape[1], M, N, K, None, epi))


def _check_pair(lib, dZ, W, X, accumulate_twice=False, label=""):
    import torch
    from test_gpu_f32x3 import x3_error_bound
    T, d_out = dZ.shape
    d_in = W.shape[0]
    assert ((T + 127) // 128) * ((d_in + 127) // 128) + ((d_in + 127) // 128) * ((d_out + 127) // 128) >= 256
    dz = _planes(lib, dZ) + ((T, d_out),)
    w = _planes(lib, W) + ((d_in, d_out),)
    x = _planes(lib, X) + ((T, d_in),)
    g = torch.Generator(device="cuda").manual_seed(77)
    dA0 = torch.randn(T, p4(d_in), device="cuda", generator=g)
    G0 = torch.randn(d_in, p4(d_out), device="cuda", generator=g)
    dA, G = dA0.clone(), G0.clone()
    reps = 2 if accumulate_twice else 1
    for _ in range(reps):
        _dual(lib, dz, w, x, dA, G, 2 if accumulate_twice else 0)
    torch.cuda.synchronize()
    # (a) against float64
    ref_a = dZ.double() @ W.double().T
    sab_a = dZ.double().abs() @ W.double().abs().T
    ref_g = X.double().T @ dZ.double()
    sab_g = X.double().abs().T @ dZ.double().abs()
    ea = float(((dA[:, :d_in].double() - ref_a).abs() / (sab_a + 1e-300)).max())
    if accumulate_twice:
        # G = fl(fl(G0 + g) + g): the contraction's own error twice + one fp32 rounding per addition at the size of its result
        want = G0[:, :d_out].double() + 2 * ref_g
        slack = 2.0 ** -24 * ((G0[:, :d_out].double() + ref_g).abs() + want.abs()) * (1 + 2.0 ** -20)
        eg = float((((G[:, :d_out].double() - want).abs() - slack).clamp(min=0) / (2 * sab_g + 1e-300)).max())
    else:
        eg = float(((G[:, :d_out].double() - ref_g).abs() / (sab_g + 1e-300)).max())
    print("%s frames %d, %d x %d: max err / sum|ab|  dA %.2e (bound %.2e)  G %.2e (bound %.2e)" % (
        label, T, d_in, d_out, ea, x3_error_bound(d_out), eg, x3_error_bound(T)))
    assert ea <= x3_error_bound(d_out), (label, T, d_in, d_out, ea)
    assert eg <= x3_error_bound(T), (label, T, d_in, d_out, eg)
    assert torch.equal(dA[:, d_in:], dA0[:, d_in:]) and torch.equal(G[:, d_out:], G0[:, d_out:])  # padding columns untouched
    # (b) against the single contractions
    sA, sG = dA0.clone(), G0.clone()
    _single(lib, 1, dz, w, sA, T, d_in, d_out, 0)
    for _ in range(reps):
        _single(lib, 2, x, dz, sG, d_in, d_out, T, 2 if accumulate_twice else 0)
    torch.cuda.synchronize()
    for name, got, single, M, N in (("dA", dA, sA, T, d_in), ("G", G, sG, d_in, d_out)):
        if _single_is_unsplit_128(M, N):
            assert torch.equal(got, single), "%s %s: the dual launch and the single contraction differ" % (label, name)
            print("  %s: bitwise equal to the single contraction" % name)
        else:
            print("  %s: the single contraction of [%d, %d] does not run unsplit 128x128 blocks -- bound only" % (name, M, N))


def _randn(shape, seed, scale=1.0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale


# (frames, d_in, d_out): cfg2's hidden layer; the output layer (2000 columns: K of dA not a multiple of 32); 255 dW tiles (an
# XCD's run of 31: one block with a single tile); M, N not multiples of 128 and K not multiples of 32; K of the grouped tiles
# below three ring tiles (64, 40: shorter than the ring -- no prefetch across the boundary), exactly three (96) and four with a
# ragged last one (100); 8192 rows (the dA tiles are the grouped ones, four per block)
SHAPES = [(1024, 2048, 2048), (1024, 2048, 2000), (1024, 2176, 1920), (1000, 2050, 2010), (64, 4096, 4096), (40, 4096, 4096),
          (96, 4096, 4096), (100, 4096, 4096), (8192, 2048, 2048)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_dual_launch_with_tile_lists(gpu, shape):
    T, d_in, d_out = shape
    _check_pair(gpu, _randn((T, d_out), 1, 3.0), _randn((d_in, d_out), 2), _randn((T, d_in), 3), label="N(0,1)")


def test_accumulating_twice(gpu):
    """epi_tn = 2 applied twice: G += g, G += g"""
    T, d_in, d_out = 1024, 2048, 2048
    _check_pair(gpu, _randn((T, d_out), 4), _randn((d_in, d_out), 5), _randn((T, d_in), 6), accumulate_twice=True, label="G += g twice")


def test_random_significands_and_adversarial_operands(gpu):
    """every one of the 24 significand bits random (all three planes carry weight), and the operands of
    test_gpu_f32x3.py::test_adversarial_operands: exponents spread over +-30 binades along rows and +-10 along k"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(21)

    def bits(rows, cols):
        m = torch.randint(1 << 23, 1 << 24, (rows, cols), device="cuda", generator=g).float() * 2.0 ** -23
        sgn = torch.randint(0, 2, (rows, cols), device="cuda", generator=g).float() * 2 - 1
        return m * sgn

    def spread(rows, cols, lo=-30, hi=30):
        x = torch.randn(rows, cols, device="cuda", generator=g)
        er = torch.randint(lo, hi + 1, (rows, 1), device="cuda", generator=g).float()
        ec = torch.randint(lo // 3, hi // 3 + 1, (1, cols), device="cuda", generator=g).float()
        return x * torch.exp2(er) * torch.exp2(ec)

    for T, d_in, d_out in [(1024, 2048, 2048), (1000, 2050, 2010)]:
        _check_pair(gpu, bits(T, d_out), bits(d_in, d_out), bits(T, d_in), label="random significands")
        _check_pair(gpu, spread(T, d_out), spread(d_in, d_out), spread(T, d_in), label="wide exponents")
