"""CPU tests of tests/kernel_check.py, the toolkit of the -m gpu kernel tests: each check must fail on the smallest violation of what it
states.  CPU tensors and fake functions only - nothing here touches a device."""

import math

import pytest
import torch

from tests import kernel_check as K

NAN = float("nan")
CPU = torch.device("cpu")


def _nan_with_payload(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_bits_tell_the_zeros_apart(dtype):
    a, b = torch.tensor([0.0, 1.0], dtype=dtype), torch.tensor([-0.0, 1.0], dtype=dtype)
    assert torch.equal(a, b) and not K.same_bits(a, b) and K.same_bits(a, a.clone())
    assert K.bits(a).dtype == {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]


def test_bits_tell_two_nan_payloads_apart():
    a, b = _nan_with_payload(0x7FC00000), _nan_with_payload(0x7FC00001)
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    assert K.same_bits(a, a.clone()) and not K.same_bits(a, b)
    assert K.same_bits(torch.tensor([3], dtype=torch.uint8), torch.tensor([3], dtype=torch.uint8))
    assert not K.same_bits(torch.tensor([3], dtype=torch.int64), torch.tensor([-3], dtype=torch.int64))


def test_worst_counts_zero_over_zero_as_zero():
    err, bound = torch.tensor([0.0, 0.5, 0.0], dtype=torch.float64), torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    assert K.worst(err, bound) == (0.5, True)
    assert K.worst(torch.tensor([1e-30], dtype=torch.float64), torch.tensor([0.0], dtype=torch.float64))[1] is False
    assert K.worst(torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)) == (0.0, True)


def test_check_bound_passes_at_the_bound_and_fails_one_ulp_outside():
    ref = torch.tensor([1.0, -2.0, 0.0, 5.0], dtype=torch.float64)
    bound = torch.tensor([0.25, 0.5, 0.0, 0.0], dtype=torch.float64)
    got = ref + torch.tensor([0.25, -0.5, 0.0, 0.0], dtype=torch.float64)   # err == bound, and 0 / 0 twice
    report = []
    assert K.check_bound(got, ref, bound, "at the bound", report) == 1.0 and report == [(1.0, "at the bound")]
    assert K.check_bound(got, ref, bound, "at the bound", exact_where_zero=True) == 1.0
    out = got.clone()
    out[0] = math.nextafter(1.25, 2.0)
    with pytest.raises(AssertionError, match=r"1 elements outside their bound.*first at \(0,\): got 1\.2500000000000002, ref 1\.0"):
        K.check_bound(out, ref, bound, "one ulp", report)
    assert len(report) == 2 and report[1][0] > 1.0   # the figure is collected before the assertion


def test_check_bound_fails_on_a_nan():
    ref = torch.zeros(2, 3, dtype=torch.float64)
    got = ref.clone()
    got[1, 2] = NAN
    with pytest.raises(AssertionError, match=r"1 non-finite outputs \(first at \(1, 2\)\)"):
        K.check_bound(got, ref, torch.full_like(ref, math.inf), "nan")
    with pytest.raises(AssertionError, match="shape"):
        K.check_bound(got[0], ref, 1.0, "shape")


def test_exact_where_zero_fails_on_one_bf16_ulp():
    ref = torch.tensor([1.0, 3.0], dtype=torch.float64)
    bound = torch.tensor([0.0, 1.0], dtype=torch.float64)
    got = torch.tensor([1.0 + 2.0 ** -7, 3.5], dtype=torch.float64)   # element 0: the next bf16 number
    with pytest.raises(AssertionError, match=r"1 of 1 decided elements are not the reference's bits \(first at \(0,\): got 1\.0078125, ref 1\.0\)"):
        K.check_bound(got, ref, bound, "decided", exact_where_zero=True)
    with pytest.raises(AssertionError, match="outside their bound"):   # without the flag the same element is simply outside its bound
        K.check_bound(got, ref, bound, "decided")
    got[0] = 1.0
    assert K.check_bound(got, ref, bound, "decided", exact_where_zero=True) == 0.5


def test_print_report(capsys):
    K.print_report([(0.25, "a"), (0.75, "b")], "title")
    K.print_report([(0.5, "c")], "other", "comparisons")
    assert capsys.readouterr().out == "title: 2 calls, worst error / bound = 0.750 (b)\nother: 1 comparisons, worst error / bound = 0.500 (c)\n"


def _nhwc_out(n=2, h=3, w=2, c=5, E=8):
    buf = K.out_buf((n, h, w), E + c + E, torch.bfloat16, 1, dev=CPU)
    buf[:n, ..., E:E + c] = 1.5
    return buf, n, c, E


def test_payload_nhwc_slice_with_a_spare_image():
    buf, n, c, E = _nhwc_out()
    assert buf.shape == (3, 3, 2, 21) and bool(torch.isnan(buf.float()[n]).all())
    out = K.payload(buf, n, c, "ok", offset=E)
    assert out.shape == (n, 3, 2, c) and out.dtype == torch.float32 and bool((out == 1.5).all())
    for where, match in (((0, 1, 1, E - 1), "outside its channel slice"), ((1, 2, 0, E + c), "outside its channel slice"),
                         ((n, 0, 0, E), "past the last image")):
        bad = buf.clone()
        bad[where] = 0.0
        with pytest.raises(AssertionError, match=match):
            K.payload(bad, n, c, "spare", offset=E)
    bad = buf.clone()
    bad[1, 0, 1, E + 2] = NAN
    with pytest.raises(AssertionError, match=r"1 non-finite outputs \(first at \(1, 0, 1, 2\)\)"):
        K.payload(bad, n, c, "nan", offset=E)


def test_payload_rows_with_spare_rows_and_fill_bytes():
    buf = K.out_buf((6,), 12, torch.float32, 4, dev=CPU)
    assert buf.shape == (10, 12)
    buf[:6, :7] = 2.0
    assert K.payload(buf, 6, 7, "ok").shape == (6, 7)
    for where, match in (((6, 0), "past the last pixel"), ((9, 11), "past the last pixel"), ((0, 7), "outside its channel slice")):
        bad = buf.clone()
        bad[where] = 7.0
        with pytest.raises(AssertionError, match=match):
            K.payload(bad, 6, 7, "spare")
    other_nan = buf.clone()
    other_nan[7, 3] = _nan_with_payload(0x7FC00001)[0]
    K.payload(other_nan, 6, 7, "any NaN is a NaN")
    with pytest.raises(AssertionError, match="past the last pixel"):
        K.payload(other_nan, 6, 7, "the very bits", exact_fill=True)
    inf = buf.clone()
    inf[0, 0] = math.inf
    assert K.payload(inf, 6, 7, "inf allowed", finite=False)[0, 0] == math.inf
    with pytest.raises(AssertionError, match="non-finite"):
        K.payload(inf, 6, 7, "inf")
    u8 = K.out_buf((2, 2, 2), 6, torch.uint8, 1, fill=255, dev=CPU)
    u8[:2, ..., 1:4] = 9
    assert K.payload(u8, 2, 3, "u8", offset=1, fill=255).dtype == torch.uint8
    u8[2, 1, 1, 5] = 254
    with pytest.raises(AssertionError, match="past the last image"):
        K.payload(u8, 2, 3, "u8", offset=1, fill=255)


def test_slice_buf_places_the_payload_and_refuses_what_the_type_cannot_hold():
    x = torch.arange(2 * 3 * 2 * 4, dtype=torch.float32).reshape(2, 3, 2, 4)
    buf = K.slice_buf(x, torch.bfloat16, 8, tail=16, fill=7.0, spare=1, lead_fill=1, dev=CPU)
    assert buf.shape == (3, 3, 2, 28) and torch.equal(buf[:2, ..., 9:12].float(), x[..., 1:])
    rest = buf.float().clone()
    rest[:2, ..., 9:12] = 7.0
    assert bool((rest == 7.0).all())
    assert bool(torch.isnan(K.slice_buf(x[0, 0], torch.float32, 4, dev=CPU)[:, :4]).all())
    front = K.slice_buf(torch.full((2, 3), 9, dtype=torch.uint8), torch.uint8, 0, tail=0, fill=255, spare=1, front=1, dev=CPU)
    assert front.shape == (4, 3) and bool((front[[0, 3]] == 255).all()) and bool((front[1:3] == 9).all())
    with pytest.raises(AssertionError, match="not representable"):
        K.slice_buf(torch.tensor([[1.0 + 2.0 ** -9]]), torch.bfloat16, 8, dev=CPU)


def test_twice_fails_on_one_bit():
    calls = []

    def steady():
        calls.append(1)
        return torch.tensor([1.0, NAN]), torch.tensor([3], dtype=torch.int64)

    assert K.twice(steady)[1].item() == 3 and len(calls) == 2
    outs = iter([torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])])
    with pytest.raises(AssertionError, match="two runs differ"):
        K.twice(lambda: next(outs), "zero sign")


def test_the_latch_is_one_per_process(monkeypatch):
    monkeypatch.setattr(K, "_FAULTED", [])
    ran = []

    @K.stop_after_fault
    def case(exc=None, value=None):
        ran.append(exc)
        if exc is not None:
            raise exc
        return value

    assert case(value=3) == 3 and case.__name__ == "case"
    with pytest.raises(AssertionError, match="a finding"):
        case(AssertionError("a finding"))
    with pytest.raises(pytest.skip.Exception):
        case(pytest.skip.Exception("skipped"))
    with pytest.raises(pytest.fail.Exception):
        case(pytest.fail.Exception("failed"))
    with pytest.raises(pytest.xfail.Exception):
        case(pytest.xfail.Exception("xfailed"))
    with pytest.raises(KeyboardInterrupt):
        case(KeyboardInterrupt())
    assert K._FAULTED == [] and case(value=4) == 4
    with pytest.raises(RuntimeError):
        case(RuntimeError("HIP error"))
    assert len(K._FAULTED) == 1 and K._FAULTED[0].startswith("tests/test_kernel_check.py::test_the_latch") and "RuntimeError" in K._FAULTED[0]
    assert "HIP error" not in K._FAULTED[0]   # the node id, not the arguments' repr
    n = len(ran)

    @K.stop_after_fault
    def another_module_s_case():
        ran.append("launched")

    for later in (case, another_module_s_case):
        with pytest.raises(AssertionError, match="not run: .* ended with an error that was no assertion"):
            later()
    assert len(ran) == n   # neither body ran


def test_payload_of_two_compares_the_sentinels_too():
    a = K.out_buf((2,), 4, torch.float32, 1, dev=CPU)
    a[:2, :3] = 1.0
    b = a.clone()
    assert K.payload_of_two((a, b), 2, 3, "same").shape == (2, 3)
    b[2, 0] = _nan_with_payload(0x7FC00001)[0]   # still a NaN, but not the first run's
    with pytest.raises(AssertionError, match="two runs differ"):
        K.payload_of_two((a, b), 2, 3, "sentinel")
