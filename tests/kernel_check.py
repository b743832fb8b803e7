"""The one toolkit of the -m gpu kernel tests (tests/test_hip_*.py that call a kernel through the C ABI and hold it to a float64 reference).

The conventions, stated once:
  inputs    the payload is a channel slice at offset E of a wider buffer (E = 16 bytes of elements: the kernels' alignment); the channels
            beside it hold a fill value - 7.0, so that a read past the slice shows as a wrong number, or NaN (the `poison` families), so
            that a neighbour's channel multiplied by a zero weight shows as NaN.  `slice_buf` builds it and asserts that the storage type
            holds the payload exactly;
  outputs   a slice of a NaN-filled buffer (`out_buf`) with spare channels beside it and spare rows - or a spare image - behind it.
            Afterwards `payload` asserts that everything outside the slice is still NaN (still the fill byte for uint8) and that the
            payload is finite.  Pitches, E, spare counts and fill values are the caller's: they are part of the layout under test;
  twice     every kernel runs two times into freshly poisoned buffers and the results agree in every bit (`twice`, `same_bits`);
  bounds    per element, from the reference's own error analysis: `check_bound` asserts `got` finite and |got - ref| <= bound element by
            element (0 / 0 counts as 0 in the reported worst share) and, with exact_where_zero, that elements whose bound is 0 carry the
            reference's bits.  No bound is tied to the largest output and none was read off a GPU run;
  faults    a failed assertion is a finding about one case.  Anything else that leaves a test (a HIP error, a refused launch) may have left
            the device in a bad state: `stop_after_fault` then fails every later decorated test of the process before it touches the device.
Plain functions; nothing here imports the GPU library until `env()` is called."""

import functools
import os

import pytest
import torch

NAN = float("nan")
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def env():
    """(DEV, L, lib, stream)"""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    return DEV, L, L.lib(), L.current_stream(DEV)


def unit_input(name, shape, lo=-1.0, hi=1.0):
    from ultralytics_pro_amd.utils import procedural as P
    return P.uniform(f"unit:{name}", shape, lo, hi)


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
def bits(t):
    """A tensor of any 1 / 2 / 4 / 8-byte element type, on the CPU or the device, as CPU integers of the same width."""
    t = t.cpu().contiguous()
    return t.view(_INT[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def twice(fn, what="two runs"):
    """fn() -> a tensor or a tuple / list of tensors, launched into buffers it poisons itself.  Runs it two times, asserts that every
    output agrees in every bit and returns the first run."""
    a, b = fn(), fn()
    la, lb = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert len(la) == len(lb), f"{what}: two runs differ in the number of outputs"
    for i, (x, y) in enumerate(zip(la, lb)):
        if isinstance(x, torch.Tensor):
            assert same_bits(x, y), f"{what}: two runs differ (output {i})"
    return a


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def worst(err, bound):
    """(max of err / bound with 0 / 0 = 0, all(err <= bound))"""
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return (float(ratio.max()) if ratio.numel() else 0.0), bool((err <= bound).all())


def _first(mask, got, ref):
    at = tuple(int(v) for v in mask.nonzero()[0])
    return f"first at {at}: got {float(got[mask][0])!r}, ref {float(ref[mask][0])!r}"


def check_bound(got, ref, bound, what, report=None, exact_where_zero=False):
    """`got` finite and |got - ref| <= bound element by element; returns the worst share of the bound and appends (share, what) to the
    list `report`, if one is given.  exact_where_zero: the share is taken over the elements with a bound above 0, and the others are
    asserted, in a statement of their own, to be the reference's very values."""
    bound = bound if isinstance(bound, torch.Tensor) else torch.full_like(ref, bound)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
    nonfinite = ~torch.isfinite(got)
    assert not bool(nonfinite.any()), (f"{what}: {int(nonfinite.sum())} non-finite outputs "
                                       f"(first at {tuple(int(v) for v in nonfinite.nonzero()[0])})")
    err = (got - ref).abs()
    zero = bound == 0
    share, ok = worst(torch.where(zero, torch.zeros_like(err), err) if exact_where_zero else err, bound)
    if report is not None:
        report.append((share, what))
    if exact_where_zero:
        bad0 = zero & (err != 0)
        assert not bool(bad0.any()), (f"{what}: {int(bad0.sum())} of {int(zero.sum())} decided elements are not the reference's bits "
                                      f"({_first(bad0, got, ref)})")
    bad = err > bound
    assert ok and not bool(bad.any()), (f"{what}: {int(bad.sum())} elements outside their bound (worst error / bound = {share:.3f}, "
                                        f"{_first(bad, got, ref) if bool(bad.any()) else 'a NaN bound'})")
    return share


def print_report(report, title, unit="calls"):
    share, what = max(report)
    print(f"{title}: {len(report)} {unit}, worst error / bound = {share:.3f} ({what})")


# ---------------------------------------------------------------------------------------------------------------------
# poisoned views
# ---------------------------------------------------------------------------------------------------------------------
def slice_buf(x, dtype, E, tail=None, fill=NAN, spare=0, front=0, lead_fill=0, dev=None):
    """CPU payload x, channels last ((rows, c) or (n, h, w, c)) -> a device buffer of `fill`, E + c + tail channels wide (tail: E) and
    `front` + `spare` rows / images longer, that holds x at [front:front + len(x), ..., E:E + c]; the first `lead_fill` channels of the
    payload stay `fill`.
    Asserts that `dtype` holds x exactly."""
    c = x.shape[-1]
    host = torch.full((front + x.shape[0] + spare,) + tuple(x.shape[1:-1]) + (E + c + (E if tail is None else tail),), fill, dtype=dtype)
    assert torch.equal(x.to(dtype).double(), x.double()), "input not representable"
    host[front:front + x.shape[0], ..., E + lead_fill:E + c] = x[..., lead_fill:].to(dtype)
    return host.to(env()[0] if dev is None else dev)


def out_buf(lead, pitch, dtype, spare, fill=NAN, dev=None):
    """A `fill`-valued device buffer (lead[0] + spare, *lead[1:], pitch): rows x pitch with spare rows, or NHWC with spare images."""
    return torch.full((lead[0] + spare,) + tuple(lead[1:]) + (pitch,), fill, dtype=dtype, device=env()[0] if dev is None else dev)


def payload(buf, n, c, what, offset=0, fill=NAN, exact_fill=False, finite=True):
    """buf: a whole output buffer (any of the layouts above) whose slice is [:n, ..., offset:offset + c].  Asserts that everything outside
    the slice still holds `fill` (NaN: any NaN, or with exact_fill the very bits `torch.full` gives) and that the slice is finite
    (finite=False: free of NaN); returns the slice on the CPU (float32 for the floating types, else the buffer's own type)."""
    a = buf.cpu()
    if exact_fill or fill == fill:
        held = bits(a) == bits(torch.full((1,), fill, dtype=a.dtype))[0]
    else:
        held = torch.isnan(a.float())
    assert bool(held[n:].all()), f"{what}: wrote past the last {'pixel' if a.dim() == 2 else 'image'}"
    assert bool(held[..., :offset].all()) and bool(held[..., offset + c:].all()), f"{what}: wrote outside its channel slice"
    out = a[:n, ..., offset:offset + c]
    if a.dtype.is_floating_point:
        out = out.float()
        nbad = ~torch.isfinite(out) if finite else torch.isnan(out)
        assert not bool(nbad.any()), f"{what}: {int(nbad.sum())} non-finite outputs (first at {tuple(int(v) for v in nbad.nonzero()[0])})"
    return out


def payload_of_two(bufs, n, c, what, **kw):
    """The output buffers of two runs of one call: identical in every bit (sentinels included), then `payload` of the first."""
    a, b = bufs
    assert same_bits(a, b), f"{what}: two runs differ"
    return payload(a, n, c, what, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the zero pass of the loss kernels (csrc/segment_train.hip ml_zero_bg_kernel, csrc/pose_train.hip kl_zero_bg_kernel)
# ---------------------------------------------------------------------------------------------------------------------
ZERO_PASS_ITEMS = 2048 * 256                 # the pass's grid cap x its workgroup: past this many 16-byte stores the grid strides
ZERO_PASS_LEVELS = ((64, 64), (8, 8), (2, 2))  # A = 4164: the levels of the cases that reach the stride


def zero_pass_items(rows, width, dtype):
    """The 16-byte stores of a zero pass over `rows` gradient rows of `width` elements of `dtype`."""
    return rows * (width // (16 // torch.empty((), dtype=dtype).element_size()))


# ---------------------------------------------------------------------------------------------------------------------
# the fault latch: one per process
# ---------------------------------------------------------------------------------------------------------------------
_FAULTED = []
_PASS_THROUGH = (AssertionError, KeyboardInterrupt, pytest.skip.Exception, pytest.xfail.Exception, pytest.fail.Exception)


def stop_after_fault(fn):
    """A failed assertion (or a skip) is about one case; anything else may have left the device in a bad state: no later decorated test
    of this process, in whatever module, launches anything then."""
    @functools.wraps(fn)
    def run(*a, **k):
        assert not _FAULTED, f"not run: {_FAULTED[0]} ended with an error that was no assertion"
        try:
            return fn(*a, **k)
        except _PASS_THROUGH:
            raise
        except BaseException as exc:
            _FAULTED.append(f"{os.environ.get('PYTEST_CURRENT_TEST', fn.__module__ + '.' + fn.__name__)}: {type(exc).__name__}")
            raise
    return run
