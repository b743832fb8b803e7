"""The training graph's rows and the planning of copy-free Concats (plain Python values: no device, no library)."""

from __future__ import annotations


class _Node:
    """One row of the model YAML inside the training graph: `op` follows the protocol of `layers` (the last node's op is the tail that
    owns the loss, `heads`); a Concat has none - it is gradient routing between nodes, the trainer's own job."""

    def __init__(self, i, f, op, cout):
        self.i, self.f, self.op, self.cout = i, f, op, cout
        self.y = None       # forward output
        self.g = None       # gradient buffer of the output


def plan_concats(rows):
    """nn.Concat without copies: a layer whose output feeds exactly one Concat writes it straight into its channel slice of the
    Concat's buffer (every kernel takes a pixel stride), and in backward that slice of the Concat's gradient IS the layer's
    gradient buffer when the Concat is the first consumer the reverse walk meets.
    rows: [(i, f, cout, can_write_in_place)] in node order; a row with a list `f` is a Concat (the only multi-input layer besides the
    tail), -1 in an `f` is the row in front.  Returns {producer index: (concat index, first channel, channels, channels of the concat)}.
    A producer gets a slot only if it appears once in that Concat's inputs, its index equals its position in `rows`, and it can write
    in place; the first Concat in node order wins; the last row (the tail) is neither planned as a Concat nor given a slot."""
    body = rows[:-1]
    cout = {i: c for i, _, c, _ in rows}
    slots = {}
    for i, f, ctot, _ in body:
        if not isinstance(f, (list, tuple)):
            continue
        idx = [j if j != -1 else i - 1 for j in f]
        c0 = 0
        for j in idx:
            if j not in slots and idx.count(j) == 1 and 0 <= j < len(body) and body[j][0] == j and body[j][3]:
                slots[j] = (i, c0, cout[j], ctot)
            c0 += cout[j]
    return slots
