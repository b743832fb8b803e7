"""Float64 CPU restatements of the attention / RT-DETR row operations behind csrc/attention.hip and csrc/transformer.hip.

Plain torch on the CPU; nothing here imports the HIP package's kernels.  tests/test_transformer_ref.py pins these functions
(against torch's own attention, the recorded MSDeformAttn golden and hand-computed clamp values); tests/test_hip_transformer.py
compares the kernels with them."""

import torch
import torch.nn.functional as F

from oracle import modules as om

F64 = torch.float64

# box_refine at and beyond the inverse_sigmoid clamps (0, eps = 1e-5, 1), crossed with these deltas
BOX_REFS = [-0.5, 0.0, 1e-6, 1e-5, 0.5, 1 - 1e-5, 1.0, 1.5]
BOX_DELTAS = [-30.0, -1.0, 0.0, 1.0, 30.0]


# ---------------------------------------------------------------------------------------------------------------------
# upa_mhsa
# ---------------------------------------------------------------------------------------------------------------------
def attention_scores(q, k, scale):
    """(q * scale) @ k^T per (image, head) in float64.  q, k: (n, L, heads, D) -> (n, heads, L, L)."""
    qh = q.to(F64).permute(0, 2, 1, 3) * float(scale)
    kh = k.to(F64).permute(0, 2, 1, 3)
    return qh @ kh.transpose(-1, -2)


def attention_ref(q, k, v, scale, residual=None):
    """softmax((q * scale) @ k^T) @ v (+ residual) per (image, head) in float64.  q, k, v, residual: (n, L, heads, D);
    every query attends to all L keys of its own (image, head).  Returns (n, L, heads, D) float64."""
    s = attention_scores(q, k, scale)
    w = torch.softmax(s, dim=-1)
    y = (w @ v.to(F64).permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    if residual is not None:
        y = y + residual.to(F64)
    return y.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# upa_layer_norm / box arithmetic / output rows
# ---------------------------------------------------------------------------------------------------------------------
def layer_norm_ref(x, residual, gamma, beta, eps):
    """F.layer_norm(x (+ residual)) over the last dim in float64."""
    z = x.to(F64) if residual is None else x.to(F64) + residual.to(F64)
    return F.layer_norm(z, (z.shape[-1],), gamma.to(F64), beta.to(F64), float(eps))


def box_refine_ref(delta, ref):
    """sigmoid(delta + inverse_sigmoid(ref)) in float64 (the oracle's inverse_sigmoid: clamp to [0, 1], eps = 1e-5)."""
    return torch.sigmoid(delta.to(F64) + om.inverse_sigmoid(ref.to(F64)))


def box_add_anchors_ref(delta, tok, anchors):
    """delta[i] + anchors[tok[i]] in the dtype of `delta` (one IEEE addition per element: float32 in, bit-exact out)."""
    return delta + anchors.to(delta.dtype)[tok.long()]


def rtdetr_output_ref(boxes, scores):
    """[boxes | sigmoid(scores)] rows in float64: (M, 4), (M, nc) -> (M, 4 + nc)."""
    return torch.cat([boxes.to(F64), torch.sigmoid(scores.to(F64))], dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# upa_msdeform_attn_strided
# ---------------------------------------------------------------------------------------------------------------------
def oracle_value_to_rows(value, shapes):
    """(bs, tokens, heads, d), tokens ordered level by level -> the kernel's level-major rows
    row(l, b, y, x) = row0[l] + (b * H_l + y) * W_l + x, as a (bs * tokens, heads * d) matrix."""
    bs, _, nh, hd = value.shape
    parts, t0 = [], 0
    for h, w in shapes:
        parts.append(value[:, t0: t0 + h * w].reshape(bs * h * w, nh * hd))
        t0 += h * w
    return torch.cat(parts, 0).contiguous()


def rows_to_oracle_value(rows, shapes, bs, heads, d):
    """Inverse of `oracle_value_to_rows`: level-major (bs * tokens, heads * d) rows -> (bs, tokens, heads, d)."""
    parts, r0 = [], 0
    for h, w in shapes:
        parts.append(rows[r0: r0 + bs * h * w].reshape(bs, h * w, heads, d))
        r0 += bs * h * w
    return torch.cat(parts, 1).contiguous()


def msdeform_ref(value_rows, shapes, bs, heads, d, offsets, logits, ref_boxes, n_points=4):
    """The oracle's multi_scale_deformable_attn in float64 on the kernel's operands.
    value_rows (bs * tokens, heads * d) level-major; offsets (bs * nq, heads * nl * np * 2) ordered (head, level, point, xy);
    logits (bs * nq, heads * nl * np); ref_boxes (bs * nq, 4) = cx, cy, w, h.  The sampling locations and weights are the ones
    the kernel is documented to form: loc = ref_xy + off / n_points * ref_wh * 0.5, w = softmax over (levels x points).
    Returns (bs * nq, heads * d) float64."""
    nl = len(shapes)
    nq = offsets.shape[0] // bs
    value = rows_to_oracle_value(value_rows.to(F64), shapes, bs, heads, d)
    so = offsets.to(F64).view(bs, nq, heads, nl, n_points, 2)
    rb = ref_boxes.to(F64).view(bs, nq, 4)
    loc = rb[:, :, None, None, None, :2] + so / n_points * rb[:, :, None, None, None, 2:] * 0.5
    aw = torch.softmax(logits.to(F64).view(bs, nq, heads, nl * n_points), -1).view(bs, nq, heads, nl, n_points)
    out = om.multi_scale_deformable_attn(value, [list(s) for s in shapes], loc, aw)
    return out.reshape(bs * nq, heads * d)
