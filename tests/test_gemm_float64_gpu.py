"""`emage_gemm` on the MI355X against float64: the case tables of tests/gemm_cases.py (the Linear grid with its epilogue features, zero-filled and
transposed tails; the convolution geometries; taps == 1 with a geometry; every product tile configuration forced onto small shapes and once at the
smallest shape where the heuristic selects it; `emage_conv_slab` against float64 and bit-equal to `emage_gemm`) through `pantomatrix_amd.ops` in F32, BF16, F16X3 and H2.  tests/test_gemm_float64_host.py runs the
same tables on the CPU, where fp32 code passes every tolerance and every wrong reference is rejected."""
import pytest
import torch

import gemm_cases as gc
from pantomatrix_amd import _lib, ops

pytestmark = pytest.mark.gpu
IDS = lambda cs: cs.ident() if isinstance(cs, gc.Case) else str(cs)


@pytest.mark.parametrize("cs", gc.LINEAR_CASES, ids=IDS)
@pytest.mark.parametrize("name", gc.DTYPES)
def test_linear(name, cs):
    gc.check_gemm(ops, name, cs)


@pytest.mark.parametrize("cs", gc.CONV_CASES, ids=IDS)
@pytest.mark.parametrize("name", gc.DTYPES)
def test_convolution_geometry(name, cs):
    gc.check_gemm(ops, name, cs)


@pytest.mark.parametrize("cs", gc.TAPS1_CASES, ids=IDS)
@pytest.mark.parametrize("name", gc.DTYPES)
def test_taps_1_with_a_geometry(name, cs):
    """include/emage_hip.h: row(m, tap) = b Lin + l stride + tap - pad holds for taps == 1 too (a strided / padded 1 x 1 convolution)."""
    gc.check_gemm(ops, name, cs)


def _forced(key, cfg, name, cases):
    """`cases` on tile configuration `cfg` of the tools library (emage_set_tuning key 0: F32 / BF16 / F16X3, key 4: H2).  No case here may be refused:
    the transposed tails start at t_col0 = bn."""
    lib = _lib.use_tools(True)
    try:
        assert lib.emage_set_tuning(key, cfg) == 0
        for cs in cases:
            gc.check_gemm(ops, name, cs)
        torch.cuda.synchronize()
    finally:
        lib.emage_set_tuning(key, -1)
        _lib.use_tools(False)


@pytest.mark.parametrize("cfg", gc.PIPE_TILES)
@pytest.mark.parametrize("name", ["f32", "bf16", "f16x3"])
def test_every_product_tile_configuration(name, cfg):
    _forced(0, cfg, name, gc.tile_cases(*gc.PIPE_TILES[cfg]))


@pytest.mark.parametrize("cfg", gc.H2_TILES)
def test_every_product_tile_configuration_h2(cfg):
    _forced(4, cfg, "h2", gc.tile_cases(*gc.H2_TILES[cfg]))


@pytest.mark.parametrize("cfg,cs", gc.HEURISTIC_PIPE, ids=IDS)
@pytest.mark.parametrize("name", ["f32", "bf16", "f16x3"])
def test_heuristic_shapes(name, cfg, cs):
    """The product library at the smallest shape where its heuristic takes configuration `cfg` in F32 / BF16 (F16X3 follows its own table)."""
    gc.check_gemm(ops, name, cs)


@pytest.mark.parametrize("cfg,cs", gc.HEURISTIC_H2, ids=IDS)
def test_heuristic_shapes_h2(cfg, cs):
    gc.check_gemm(ops, "h2", cs)


@pytest.mark.parametrize("cs", gc.SLAB_CASES, ids=IDS)
@pytest.mark.parametrize("name", gc.SLAB_DTYPES)
def test_conv_slab(name, cs):
    """`emage_conv_slab` against float64 at the block edges of its 128-position tile, and still bit-identical to `emage_gemm`."""
    gc.check_conv_slab(ops, name, cs)


@pytest.mark.parametrize("case", gc.WAV_CASES, ids=str)
@pytest.mark.parametrize("name", gc.WAV_DTYPES)
def test_wav_conv_in(name, case):
    gc.check_wav_conv_in(ops, name, *case)


@pytest.mark.parametrize("nclip,nwin", gc.BLOCK0_CASES)
@pytest.mark.parametrize("name", gc.BLOCK0_DTYPES)
def test_wav_block0(name, nclip, nwin):
    gc.check_wav_block0(ops, name, nclip, nwin)


def test_bad_geometry_is_refused():
    """Argument checks of csrc/gemm.hip `make_args`, which run before any launch: pad < 0 (it would wrap the base of A's buffer descriptor), and the
    LayerNorm fold on anything but the plain Linear geometry (its statistics are indexed by the output row)."""
    a = torch.zeros(24, 64, device="cuda")
    w = torch.zeros(64, 64, device="cuda")
    out = torch.full((24, 64), 7.0, device="cuda")
    for name, dtype in gc.DTYPES.items():
        with pytest.raises(_lib.EmageKernelError, match="EINVAL"):
            ops.gemm(dtype, a.to(ops.TORCH_DTYPE[dtype]), w.to(ops.TORCH_DTYPE[dtype]), None, None, None, out.to(ops.TORCH_DTYPE[dtype]), None, None,
                     n=64, cp=64, taps=1, stride=1, pad=-1, lin=8, lout=8, m=24)
    stats, c = torch.zeros(24, 24, 2, device="cuda"), torch.zeros(768, device="cuda")
    a, w, out = torch.zeros(24, 768, device="cuda"), torch.zeros(768, 768, device="cuda"), torch.full((24, 768), 7.0, device="cuda")
    with pytest.raises(_lib.EmageKernelError, match="EINVAL"):
        ops.gemm(gc.H2, a, w, c, None, None, out, None, None, n=768, cp=768, taps=1, stride=2, pad=0, lin=16, lout=8, m=8, ln=(stats, c))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
