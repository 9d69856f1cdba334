"""The case tables of tests/gemm_cases.py run on the CPU: through the fp32 stand-in `fake_ops.gemm` in all four dtypes, and for the F32 rows through
torch's own fp32 `F.linear` / `F.conv1d` behind the `gemm` signature.  Correct fp32 code passes every tolerance the GPU test applies, every wrong
reference is rejected by more than FAR x the tolerance (asserted inside `check_gemm`), and the input conditions the cases rely on hold: the margin
of the rows scaled 1e3 below the fp16 range, the cancelling rows, the outputs that see only padding.  No GPU."""
import pytest
import torch

import fake_ops as F
import gemm_cases as gc
from pantomatrix_amd import ops

IDS = lambda cs: cs.ident() if isinstance(cs, gc.Case) else str(cs)
SMALL = gc.LINEAR_CASES + gc.CONV_CASES + gc.TAPS1_CASES


@pytest.mark.parametrize("cs", SMALL, ids=IDS)
@pytest.mark.parametrize("name", gc.DTYPES)
def test_gemm(name, cs):
    gc.check_gemm(F, name, cs)


class TorchGemm:
    """torch's own fp32 Linear / Conv1d on the CPU behind the `gemm` signature (F32 only): `F.linear` for the identity geometry, else `F.conv1d` on
    the (nb, Cp, Lin) tensor, padded by hand where the geometry asks for more output positions than torch's formula gives."""

    @staticmethod
    def gemm(dtype, a, w, bias=None, slope=None, res=None, out=None, out_f32=None, out_t=None, *, n, cp, n_store=0, t_col0=0, t_rows=0,
             res_first=False, taps=1, stride=1, pad=0, lin=None, lout=None, m=None, w_scale=1.0, res_h2=False):
        assert dtype == gc.F32 and not res_h2
        nb = m // lout
        x = torch.as_strided(a, (nb * lin, cp), (a.stride(0), 1))
        if taps == 1 and stride == 1 and pad == 0 and lin == lout:
            v = torch.nn.functional.linear(x, w)
        else:
            right = max(0, (lout - 1) * stride + taps - pad - lin)
            xp = torch.nn.functional.pad(x.view(nb, lin, cp).transpose(1, 2), (pad, right))
            v = torch.nn.functional.conv1d(xp, w.view(n, taps, cp).transpose(1, 2), stride=stride)[:, :, :lout].transpose(1, 2).reshape(m, n)
        if bias is not None:
            v = v + bias
        rv = torch.as_strided(res, (m, n), (res.stride(0), 1)) if res is not None else None
        if rv is not None and res_first:
            v = v + rv
        if slope is not None:
            v = torch.where(v > 0, v, v * slope)
        if rv is not None and not res_first:
            v = v + rv
        ncol = n if out_t is None else t_col0
        if out is not None:
            out[:, :ncol] = v[:, :ncol]
            out[:, n:max(n, n_store)] = 0
        if out_f32 is not None:
            out_f32[:, :ncol] = v[:, :ncol]
        if out_t is not None:
            out_t[:, :, :t_rows] = v[:, t_col0:].reshape(m // t_rows, t_rows, n - t_col0).permute(0, 2, 1)


@pytest.mark.parametrize("cs", SMALL, ids=IDS)
def test_gemm_torch_fp32(cs):
    gc.check_gemm(TorchGemm, "f32", cs)


@pytest.mark.parametrize("cfg", list(gc.PIPE_TILES) + list(gc.H2_TILES))
def test_tile_configuration_cases(cfg):
    """The small shapes every product tile configuration is forced onto."""
    for name in (("h2",) if cfg in gc.H2_TILES else ("f32", "bf16", "f16x3")):
        for cs in gc.tile_cases(*(gc.H2_TILES if cfg in gc.H2_TILES else gc.PIPE_TILES)[cfg]):
            gc.check_gemm(F, name, cs)


@pytest.mark.parametrize("cfg,cs", gc.HEURISTIC_PIPE + gc.HEURISTIC_H2, ids=IDS)
def test_heuristic_shape_cases(cfg, cs):
    for name in (("h2",) if cfg in gc.H2_TILES else ("f32", "bf16", "f16x3")):
        gc.check_gemm(F, name, cs)


def test_heuristic_shapes_select_their_configuration():
    """csrc/gemm.hip `dispatch` (F32 / BF16) and csrc/gemm_h2.hip `h2_config_for` on 256 CUs, restated: each shape is the one the table says."""
    tiles = lambda m, n, bm, bn: ((m + bm - 1) // bm) * ((n + bn - 1) // bn)

    def pipe(cs):
        if cs.taps >= 15 and cs.m > 8192:
            return 36
        if cs.n > 64 and tiles(cs.m, cs.n, 128, 128) >= 512:
            return 34
        if cs.n % 192 == 0 and ((cs.m + 63) // 64) * (cs.n // 192) == 512:
            return 33
        if cs.taps == 1 and cs.n == 768 and cs.m >= 2048:
            return 32
        return 25

    def h2(cs):
        if cs.n >= 1024 and cs.m >= 1024:
            if tiles(cs.m, cs.n, 128, 192) >= 4 * 256 and cs.n % 192 == 0:
                return 170
            if tiles(cs.m, cs.n, 128, 256) >= 2 * 256 and cs.n % 256 == 0:
                return 119
            return 100 if cs.n % 192 == 0 else 113
        return 120

    for cfg, cs in gc.HEURISTIC_PIPE:
        assert pipe(cs) == cfg, (cfg, cs)
    for cfg, cs in gc.HEURISTIC_H2:
        assert h2(cs) == cfg, (cfg, cs)
    for cs in SMALL:
        assert pipe(cs) == 25 and h2(cs) == 120


def test_input_conditions():
    """What the cases promise about their inputs."""
    for cs in (c for c in gc.LINEAR_GRID if c.kinds):
        for name in gc.DTYPES:
            inp = gc.inputs(name, cs)
            a = inp["a"][:, :cs.c]
            kind = torch.arange(cs.m) % 5
            assert float(inp["a"].abs().max()) * ops.A_SCALE_F16X3 < 65504, "the fp16 hi plane of a * 16 stays finite"
            assert float(a[kind == 2].abs().max()) > 1e3 and float(a[kind == 1].abs().max()) < 1e-3
            assert not bool(a[kind == 4].any())
            if cs.c < cs.cp:
                assert bool((inp["a"][:, cs.c:] == gc.TAIL).all()) and not bool(inp["w"][:, :, cs.c:].any())
            r = gc.reference(name, cs, torch.arange(cs.m))
            ratio = (r["s"] / r["v"].abs().clamp_min(1e-300))[kind == 3].median()
            print(f"{cs.tag(name)}: cancelling rows: median S / |v| = {float(ratio):.1f}")
            assert float(ratio) > 1e3, "S is at least 1e3 x |v| on the cancelling rows, in every dtype (bf16, whose stored row is coarser, included)"
            assert bool((r["s"][kind == 4] == 0).all()) and bool((r["floors"][kind == 4] == 0).all()), "an all-zero row has a zero contraction tolerance"
    seen = 0
    for cs in gc.CONV_CASES:
        dead = gc.pad_only_rows(cs)
        if (cs.taps, cs.stride, cs.pad, cs.lin, cs.lout) == gc.PAD_ONLY:
            assert int(dead.sum()) == 4 * cs.nb
            r = gc.reference("h2", cs, torch.arange(cs.m))
            assert bool((r["s"][dead] == 0).all()) and bool((r["floors"][dead] == 0).all())
            seen += 1
        if cs.loud:
            inp = gc.inputs("f32", cs)
            seq = torch.arange(cs.nb * cs.lin) // cs.lin
            assert cs.nb == 3 and float(inp["a"][seq != 1, :cs.c].abs().median()) > 100 * float(inp["a"][seq == 1, :cs.c].abs().median())
            assert float(inp["a"].abs().max()) * ops.A_SCALE_F16X3 < 65504
    assert seen == 2
    assert any(c.lout == 37 and c.nb == 3 for c in gc.CONV_CASES), "a 64-row tile spans a sequence boundary"


@pytest.mark.parametrize("cs", gc.SLAB_CASES, ids=IDS)
@pytest.mark.parametrize("name", gc.SLAB_DTYPES)
def test_conv_slab(name, cs):
    gc.check_conv_slab(F, name, cs)


@pytest.mark.parametrize("case", gc.WAV_CASES, ids=str)
@pytest.mark.parametrize("name", gc.WAV_DTYPES)
def test_wav_conv_in(name, case):
    gc.check_wav_conv_in(F, name, *case)


@pytest.mark.parametrize("nclip,nwin", gc.BLOCK0_CASES)
@pytest.mark.parametrize("name", gc.BLOCK0_DTYPES)
def test_wav_block0(name, nclip, nwin):
    gc.check_wav_block0(F, name, nclip, nwin)
