"""CPU (-m "not gpu"): the float64 references of tests/transformer_ref.py are themselves right - against torch's own
scaled-dot-product attention, the recorded MSDeformAttn golden and hand-computed values at the inverse_sigmoid clamps."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import modules as om
from tests import transformer_ref as TR
from tests.kernel_check import unit_input
from ultralytics_pro_amd.utils import procedural as P


@pytest.mark.parametrize("n,L,heads,D,scale", [(2, 5, 3, 4, 1.0), (1, 65, 2, 32, 32 ** -0.5), (2, 17, 4, 16, 0.25)])
def test_attention_ref_matches_torch_sdpa(n, L, heads, D, scale):
    g = torch.Generator().manual_seed(L * 100 + D)
    q, k, v, r = (torch.rand(n, L, heads, D, generator=g, dtype=torch.float64) * 4 - 2 for _ in range(4))
    want = F.scaled_dot_product_attention(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), scale=scale).permute(0, 2, 1, 3)
    got = TR.attention_ref(q, k, v, scale)
    assert got.dtype == torch.float64 and got.shape == (n, L, heads, D)
    assert float((got - want).abs().max()) <= 1e-13
    assert float((TR.attention_ref(q, k, v, scale, r) - (want + r)).abs().max()) <= 1e-13
    # float32 operands are promoted, not computed in float32
    got32 = TR.attention_ref(q.float(), k.float(), v.float(), scale)
    assert got32.dtype == torch.float64
    s = TR.attention_scores(q, k, scale)
    assert s.shape == (n, heads, L, L)
    assert float((s[0, 1, 2, 3] - scale * (q[0, 2, 1] * k[0, 3, 1]).sum()).abs()) <= 1e-13


def test_attention_ref_keeps_images_and_heads_apart():
    """v constant per (image, head): the output is that constant whatever q and k are."""
    g = torch.Generator().manual_seed(3)
    n, L, heads, D = 2, 9, 3, 8
    q, k = (torch.rand(n, L, heads, D, generator=g) * 6 - 3 for _ in range(2))
    c = torch.arange(1, n * heads + 1, dtype=torch.float32).view(n, 1, heads, 1)
    y = TR.attention_ref(q, k, c.expand(n, L, heads, D), 0.7)
    assert float((y - c.double()).abs().max()) <= 1e-14


def test_msdeform_ref_matches_golden(golden_dir):
    """`msdeform_ref` on the operands MSDeformAttn(32, 3, 4, 4) forms (built as test_oracle_golden.py builds it), through
    the level-major row layout, reproduces the reference's recorded output."""
    G = np.load(golden_dir / "ops_unit.npz")
    o = om.MSDeformAttn(32, 3, 4, 4).eval()
    P.apply_procedural_weights(o)
    o = o.double()
    shapes = [[8, 8], [4, 4], [2, 2]]
    bs, nq, heads, d = 2, 10, 4, 8
    query = unit_input("msda_q", (bs, nq, 32)).double()
    ref_b = unit_input("msda_ref", (bs, nq, 1, 4), 0.1, 0.9).double()
    val = unit_input("msda_v", (bs, 84, 32)).double()
    with torch.no_grad():
        value = o.value_proj(val).view(bs, 84, heads, d)
        rows = TR.oracle_value_to_rows(value, shapes)
        assert rows.shape == (bs * 84, 32)
        assert torch.equal(TR.rows_to_oracle_value(rows, shapes, bs, heads, d), value)
        # level-major: image 1's first 8x8 token follows image 0's last 8x8 token
        assert torch.equal(rows[64], value[1, 0].reshape(-1)) and torch.equal(rows[128], value[0, 64].reshape(-1))
        off = o.sampling_offsets(query).reshape(bs * nq, -1)
        lg = o.attention_weights(query).reshape(bs * nq, -1)
        y = TR.msdeform_ref(rows, shapes, bs, heads, d, off, lg, ref_b.reshape(bs * nq, 4))
        assert y.dtype == torch.float64 and y.shape == (bs * nq, 32)
        y = o.output_proj(y).view(bs, nq, 32)
    assert np.abs(y.numpy() - G["msdeform_attn"]).max() <= 1e-5


def test_msdeform_ref_far_outside_is_exactly_zero():
    g = torch.Generator().manual_seed(5)
    shapes = [(5, 7), (1, 1)]
    bs, nq, heads, d = 1, 3, 2, 8
    rows = torch.rand(bs * 36, heads * d, generator=g)
    off = torch.full((bs * nq, heads * 2 * 4 * 2), 3e9)
    off[:, ::3] = -1e6
    lg = torch.zeros(bs * nq, heads * 2 * 4)
    ref = torch.tensor([[0.5, 0.5, 0.25, 0.5]]).repeat(bs * nq, 1)
    y = TR.msdeform_ref(rows, shapes, bs, heads, d, off, lg, ref)
    assert bool((y == 0).all())


REFS, DELTAS = TR.BOX_REFS, TR.BOX_DELTAS


def test_box_refine_ref_at_the_clamps():
    """sigmoid(d + log(a / b)) = a e^d / (a e^d + b) with a = max(clamp(x), eps), b = max(1 - clamp(x), eps), eps = 1e-5:
    worked by hand in Python floats for every (reference, delta) pair the GPU test uses."""
    eps = 1e-5
    ref = torch.tensor(REFS, dtype=torch.float64).repeat_interleave(len(DELTAS))
    dl = torch.tensor(DELTAS, dtype=torch.float64).repeat(len(REFS))
    got = TR.box_refine_ref(dl, ref)
    for i in range(ref.numel()):
        x = min(max(float(ref[i]), 0.0), 1.0)
        a, b = max(x, eps), max(1.0 - x, eps)
        e = math.exp(float(dl[i]))
        want = a * e / (a * e + b)
        assert abs(float(got[i]) - want) <= 1e-15 + 1e-12 * want, (float(ref[i]), float(dl[i]), float(got[i]), want)
    # the clamps themselves, with no delta: below 0 = 0; under eps the numerator is eps; above 1 = 1
    z = TR.box_refine_ref(torch.zeros(8, dtype=torch.float64), torch.tensor(REFS, dtype=torch.float64))
    lo, hi = 1e-5 / (1 + 1e-5), 1 / (1 + 1e-5)
    want = torch.tensor([lo, lo, 1e-5 / (1e-5 + (1 - 1e-6)), 1e-5, 0.5, 1 - 1e-5, hi, hi], dtype=torch.float64)
    assert float((z - want).abs().max()) <= 1e-15


def test_row_refs():
    g = torch.Generator().manual_seed(9)
    x, r = torch.randn(6, 100, generator=g) + 30, torch.randn(6, 100, generator=g)
    gamma, beta = torch.rand(100, generator=g) + 0.5, torch.randn(100, generator=g)
    y = TR.layer_norm_ref(x, r, gamma, beta, 1e-3)
    z = x.double() + r.double()
    want = (z - z.mean(-1, keepdim=True)) / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + 1e-3) * gamma.double() + beta.double()
    assert y.dtype == torch.float64 and float((y - want).abs().max()) <= 1e-12
    anchors = torch.tensor([[0.0, 1, 2, 3], [float("inf")] * 4, [4, 5, 6, 7]])
    d = torch.ones(3, 4)
    out = TR.box_add_anchors_ref(d, torch.tensor([2, 1, 0], dtype=torch.int32), anchors)
    assert out.dtype == torch.float32 and out.tolist() == [[5, 6, 7, 8], [float("inf")] * 4, [1, 2, 3, 4]]
    o = TR.rtdetr_output_ref(torch.tensor([[0.1, 0.2, 0.3, 0.4]]), torch.tensor([[0.0, 200.0, -800.0]]))
    assert o.shape == (1, 7) and o[0, 4:].tolist() == [0.5, 1.0, 0.0]
    assert torch.equal(o[0, :4].float(), torch.tensor([0.1, 0.2, 0.3, 0.4]))
