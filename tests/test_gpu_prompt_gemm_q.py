"""The tiled prompt GEMMs' code-reading forms (conv_gemm_kernel / conv_gemm2_kernel WM 1 / 2, fm_codec_kernels.hip)
through fm_op_prompt_gemm_q: the hook quantises a bf16-valued weight on the device with the model's rule, packs the
bf16 fragments and the step-granular codes with the model's pack launchers, and runs launch_conv_gemm -- the call the
prompt pass makes for a quantised linear of more than 64 rows (fm_tune prompt_gemm_q) -- once per form on the same
rows.  The code forms rebuild every bf16 fragment bit for bit and keep mode 0's plan (kernel, K slices, row segments)
and epilogues, so the two outputs are compared with array_equal; the bf16 form's output is then held to
test_gpu_linear_ops.py's bounds (its docstring derives them) of the float64 product over the dequantised codes the hook
returns, carried through the epilogue's rounding chain: int8 round(round(sum) * scale[row]) (v_q8), + bias, the
rounding, then round(res + y).  The bit-exact shares against the restatement are printed, not held (no floor is
recorded for these families).  Every case asserts the plan the hook returns, so each kernel is known to have run.

Shapes: the smallest at which each form can go wrong.  Register kernel (64 x 64 tiles): R 65 / 100 (a ragged second
row tile), N 96 / 112 (a 64-wide block with one wave's channels only, and its second channel tile absent) / 272, K 128
(one int4 unit), 160 (int8: 5 steps, the tail of the 4-step unroll), 384 whole and in 2 / 4 slices, 1152 in 4 slices
of 9 steps (slices start 1, 2 and 3 steps into a 128-k unit: the int4 unit selection); ksplit 1 is the kernel's own
epilogue with the row scales.  LDS8 (128 rows x 128 channels): N 2048, R 129 / 200, K 512 in 8 slices (2 x 16 x 8 =
256 blocks, conv_kernel_of's threshold), and unsplit -- cg_epilogue with the row scales -- at N 16384, R 257, K 128
(3 x 128 blocks).  LDS6 (96 channels): N 272, R 1024, K 512 in 16 one-step slices (8 x 3 x 16 blocks); N 272's last
column block holds 5 of its 6 channel tiles, so N 208 (8 x 2 x 16 = 256 blocks) is run beside it for the block with
one tile; unsplit (Lq >= 4096 plans the LDS kernel whatever the grid) at N 208, R 4096, K 128.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from fishmi import ops
from linear_ref import mk as _mk, v_acc, v_add, v_q8, v_rnd
from test_gpu_linear_ops import _buf, _check, _same, _sentinel
from test_gpu_prompt_skinny_q import _dequant, _weights

QUANTS = [("int8", 128), ("int4", 128), ("int4", 256)]
CEK_GEMM, CEK_SPLITK = 0, 1
EPIS = ("store", "bias", "resid")


def _case(quant, gs, R, N, K, ksplit, epi, kernel):
    rng = np.random.default_rng(R + N + K + gs + 7 * ksplit)
    ldx, ld = K + 8, N + 8
    w, x = _weights(rng, N, K, quant), _mk(rng, (R, ldx), "bf16")
    bias = _mk(rng, (N,), "bf16") if epi != "store" else None
    res = _mk(rng, (R, ld), "bf16") if epi == "resid" else None
    tag = f"gemm_q {quant} gs={gs} R={R} N={N} K={K} ks={ksplit} {epi}"
    outs = []
    for reps in (1, 3):
        yq, yb = _buf(R + 2, ld), _buf(R + 2, ld)
        plan, q, sc, zr = ops.prompt_gemm_q(w, x, yq, yb, quant, gs=gs, bias=bias, res=res, ksplit=ksplit, reps=reps)
        want = {"kernel": kernel, "ksplit": ksplit, "nseg": 1, "epi": CEK_SPLITK if ksplit > 1 else CEK_GEMM,
                "seg_rows": R, "kernel_last": kernel}
        assert plan == want, (tag, plan)
        _same(f"{tag} reps={reps}: codes vs bf16 fragments", yq, yb)
        _sentinel(tag, yq, R, N)
        _sentinel(tag, yb, R, N)
        outs.append(yb)
    _same(tag + " reps 3 vs 1", outs[0], outs[1])
    lo, hi = (-128, 127) if quant == "int8" else (0, 15)
    assert q.min() == lo and q.max() == hi, (tag, int(q.min()), int(q.max()))
    v = v_acc(x[:, :K], _dequant(quant, q, sc, zr))
    if quant == "int8":
        v = v_q8(v, sc[None, :].astype(np.float64), "bf16")
    if bias is not None or quant != "int8":  # (int8 without a bias: the second rounding changes nothing)
        v = v_rnd(v_add(v, None if bias is None else bias[None, :].astype(np.float64)), "bf16")
    if res is not None:
        v = v_rnd(v_add(v, res[:, :N].astype(np.float64)), "bf16")
    _check(tag, f"gemm_q/{quant}/{'split' if ksplit > 1 else 'direct'}", outs[0][:R, :N], v)


# (K, ksplit); K = 160 is no whole int4 unit
REG_PLANS = [(128, 1), (160, 1), (384, 1), (384, 2), (384, 4), (1152, 4)]
REG_CASES = [(q, gs, K, ks) for q, gs in QUANTS for K, ks in REG_PLANS if q == "int8" or K % gs == 0]


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs,K,ksplit", REG_CASES)
def test_register_kernel(quant, gs, K, ksplit):
    """conv_gemm_kernel: R 65 / 100 x N 96 / 112 / 272, each with store, bias and residual"""
    for R in (65, 100):
        for N in (96, 112, 272):
            for epi in EPIS:
                _case(quant, gs, R, N, K, ksplit, epi, ops.CK_REG)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs", QUANTS)
def test_lds8_split(quant, gs):
    """conv_gemm2_kernel<8>, 8 K slices: two row tiles (the second ragged) x 16 column tiles"""
    for R, epi in ((129, "store"), (200, "resid")):
        _case(quant, gs, R, 2048, 512, 8, epi, ops.CK_LDS8)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs", QUANTS[:2])
def test_lds8_direct(quant, gs):
    """conv_gemm2_kernel<8> unsplit: cg_epilogue, with the int8 row scales (K = 128 is no whole group of 256)"""
    _case(quant, gs, 257, 16384, 128, 1, "resid", ops.CK_LDS8)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs", QUANTS)
def test_lds6_split(quant, gs):
    """conv_gemm2_kernel<6>, 16 one-step slices: a last column block of 5 channel tiles (N 272) and of 1 (N 208)"""
    _case(quant, gs, 1024, 272, 512, 16, "resid", ops.CK_LDS6)
    _case(quant, gs, 1024, 208, 512, 16, "bias", ops.CK_LDS6)


@pytest.mark.gpu
@pytest.mark.parametrize("quant,gs", QUANTS[:2])
def test_lds6_direct(quant, gs):
    """conv_gemm2_kernel<6> unsplit (4096 rows): cg_epilogue, with the int8 row scales"""
    _case(quant, gs, 4096, 208, 128, 1, "resid", ops.CK_LDS6)


def test_refusals():
    """FM_ERR_ARG before any device call: int4 outside whole 128-k units, more slices than k-steps, a short output"""
    from fishmi import native

    rng = np.random.default_rng(1)
    w, x = _mk(rng, (96, 160), "bf16"), _mk(rng, (65, 160), "bf16")
    for kw, shape in ((dict(quant="int4"), (65, 96)), (dict(quant="int8", ksplit=6), (65, 96)),
                      (dict(quant="int8"), (64, 96)), (dict(quant="int8"), (65, 88))):
        with pytest.raises(native.FishMIError) as e:
            ops.prompt_gemm_q(w, x, _buf(*shape), _buf(*shape), **kw)
        assert e.value.code == -1
