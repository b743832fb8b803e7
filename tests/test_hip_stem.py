"""-m gpu: every kernel instantiation csrc/stem.hip can launch - the scalar stem_conv_kernel, stem_mfma_kernel with its POOL and G16 forms,
stem_conv_fused_kernel<4 | 8, 3 | 6>, stem_conv_fused32_kernel<1 | 2> - through the C ABI against the float64 reference of
tests/stem_ref.py, element by element: inside the reference's bound everywhere, and BIT-EQUAL to the reference's bf16 value wherever that
bound is 0 (98 to 99 % of a fused case's outputs on `positive`).  All tolerances are conv_ref.conv_bound / block_ref.stage: none is tied
to the largest output and none was read off a GPU run.

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py.
The input is images [1, 1 + n) of an (n + 2)-image NaN-filled (uint8: 255-filled) allocation, the output a channel slice at offset 8 with a spare image behind;
every case first asserts, through upa_stem_variant / upa_stem_fused_variant, the family, instantiation, staging form, waves and workgroup
count it dispatches to (and workgroups < tiles where it is meant to walk several tiles per workgroup).

Each case prints its worst |kernel - ref| / bound; STEM_STATS=1 adds the share of outputs held bit-exact."""

import ctypes as C
import os

import pytest
import torch

from tests import stem_ref as S
from tests.conv_ref import ACT_NONE, ACT_RELU, ACT_SILU
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

E = 8  # spare channels in front of the output slice (16 bytes of bf16: the kernels' store alignment)
NAN = float("nan")
XCODE = {"f32": 0, "bf16": 1, "u8": 2}   # UPA_F32, UPA_BF16, UPA_U8_BGR_HWC
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
EINVAL, EUNSUPPORTED = -1, -2


def _opts(case_opts):
    """The case's `upa_opts` switches on top of the session's options."""
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    base = R.current_opts()
    return base.replace(**case_opts) if base is not None else L.Opts(**case_opts)


def _dev_input(x, fmt, misalign=False):
    """CPU payload -> (pointer to image 1 of an (n + 2)-image poisoned device allocation, the allocation).  misalign: the whole allocation
    starts 2 bytes into its buffer."""
    from tests.hip_utils import DEV
    host = KC.slice_buf(x, torch.uint8 if fmt == "u8" else TORCH[fmt], 0, tail=0, fill=255 if fmt == "u8" else NAN, spare=1, front=1, dev="cpu")
    per = host[0].numel() * host.element_size()
    if misalign:
        assert fmt == "bf16"
        flat = torch.full((host.numel() + 8,), NAN, dtype=torch.bfloat16)
        flat[1:1 + host.numel()] = host.flatten()
        dev = flat.to(DEV)
        ptr = dev.data_ptr() + 2 + per
        assert ptr % 16 == (2 + per) % 16
    else:
        dev = host.to(DEV)
        ptr = dev.data_ptr() + per
    return ptr, dev


def _out(n, c, oh, ow, dtype):
    """(the NaN-filled output buffer with a spare image, the pointer to its channel slice at E, its pitch)"""
    ld = E + c + E + (-c % 8)
    buf = KC.out_buf((n, oh, ow), ld, dtype, 1)
    return buf, buf.data_ptr() + E * buf.element_size(), ld


def _held(buf, n, c, ref, e, what):
    """Nothing outside the slice written; inside the bound everywhere, and where the bound is 0 the reference's bits."""
    got = KC.payload(buf, n, c, what, offset=E).permute(0, 3, 1, 2).to(torch.float64)
    share = KC.check_bound(got, ref, e, what, exact_where_zero=True)
    print(f"STEM {what}: worst |d| / bound = {share:.4f}", flush=True)
    if os.environ.get("STEM_STATS"):
        print(f"STEM_STATS {what}|exact={float((e == 0).double().mean()):.4f}|worst_share={share:.4f}", flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# upa_conv2d_stem_nchw / upa_conv2d_stem_nchw_pool2
# ---------------------------------------------------------------------------------------------------------------------
def _run_single(case, d, pk):
    """Assert the dispatch, launch once into fresh poisoned buffers -> the whole output buffer on the CPU."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    n, cout = case["n"], case["cout"]
    pool = case["pool"]
    oh, ow = (case["oh"] // 2, case["ow"] // 2) if pool else (case["oh"], case["ow"])
    xptr, keep = _dev_input(d["x"], case["fmt"], case["misalign"])
    odt = TORCH[case["out"]]
    buf, yptr, ld = _out(n, cout, oh, ow, odt)
    opts = _opts(case["opts"])
    args = (XCODE[case["fmt"]], n, case["cin"], case["h"], case["w"])
    tail = (cout, ld, case["k"], case["s"], case["pad"], case["act"], L.dtype_code(odt))
    v = lib.upa_stem_variant(*args, *tail, pool, C.byref(opts), xptr & 15)
    assert v >= 0, f"upa_stem_variant refused: {v}"
    got = S.decode_variant(v)
    assert got == case["expect"], (got, case["expect"])   # before anything is launched
    if case["walk"]:
        assert got["wgs"] < case["tiles"]
    if case["misalign"]:
        assert xptr % 16 == 2 and got["staging"] == S.VGPR
    fn = lib.upa_conv2d_stem_nchw_pool2 if pool else lib.upa_conv2d_stem_nchw
    rc = fn(xptr, *args, pk.w.data_ptr(), pk.bias.data_ptr(), yptr, *tail, C.byref(opts), L.current_stream(DEV))
    L.check(rc, "stem")
    torch.cuda.synchronize()
    return buf.cpu()


def _single_test(kind, index):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    case = (S.SINGLE_CASES if kind == "single" else S.POOL_CASES)[index]
    d, (ref, bound) = S.single_case_reference(kind, index)
    pk = PackedConv(d["w"], d["b"], case["k"], DEV, torch.float32, True)
    _held(KC.twice(lambda: _run_single(case, d, pk)), case["n"], case["cout"], ref, bound, case["id"])


@pytest.mark.parametrize("index", range(len(S.SINGLE_CASES)), ids=[c["id"] for c in S.SINGLE_CASES])
@KC.stop_after_fault
def test_stem_kernel_vs_f64(index):
    _single_test("single", index)


@pytest.mark.parametrize("index", range(len(S.POOL_CASES)), ids=[c["id"] for c in S.POOL_CASES])
@KC.stop_after_fault
def test_stem_pool_kernel_vs_f64_chain(index):
    _single_test("pool", index)


# ---------------------------------------------------------------------------------------------------------------------
# upa_stem_conv_fused_s
# ---------------------------------------------------------------------------------------------------------------------
def _fused_args(case):
    return (case["n"], case["h"], case["w"], case["k0"], case["s0"], case["c0"])


def _run_fused(case, d, pa, pb):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    n, c = case["n"], 2 * case["c0"]
    xptr, keep = _dev_input(d["x"], "bf16")
    buf, yptr, ld = _out(n, c, case["oh"], case["ow"], torch.bfloat16)
    opts = _opts(case["opts"])
    v = lib.upa_stem_fused_variant(*_fused_args(case), ld, C.byref(opts), xptr & 15)
    assert v >= 0, f"upa_stem_fused_variant refused: {v}"
    got = S.decode_variant(v)
    assert got == case["expect"], (got, case["expect"])
    if case["walk"]:
        assert got["wgs"] < case["tiles"]
    rc = lib.upa_stem_conv_fused_s(xptr, *_fused_args(case), pa.w.data_ptr(), pa.bias.data_ptr(), pb.w.data_ptr(), pb.bias.data_ptr(), yptr, ld,
                                   C.byref(opts), L.current_stream(DEV))
    L.check(rc, "stem_conv_fused")
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("index,family", [pytest.param(i, f, id=f"{c['id']}-{f}") for i, c in enumerate(S.FUSED_CASES) for f in c["families"]])
@KC.stop_after_fault
def test_fused_stem_pair_vs_f64_chain(index, family):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    case = S.FUSED_CASES[index]
    d, (ref, e) = S.fused_case_reference(index, family)
    pa = PackedConv(d["w0"], d["b0"], case["k0"], DEV, torch.bfloat16, True)
    pb = PackedConv(d["w1"], d["b1"], 3, DEV, torch.bfloat16, False)
    _held(KC.twice(lambda: _run_fused(case, d, pa, pb)), case["n"], 2 * case["c0"], ref, e, f"{case['id']}-{family}")


def test_the_cases_name_every_instantiation_the_file_can_launch():
    """What the cases above ASSERT of the dispatch query covers stem.hip's launch sites: scalar x {f32, bf16} x {SiLU, none}, mfma x NT x (KS, S)
    x {SiLU, none} + G16 / POOL / G16 POOL per NT, fused16 x {8 waves, 4 waves, k0 6}, fused32 x {stride 2, 1}."""
    met = {S.instantiation(c["expect"]) for c in S.SINGLE_CASES + S.POOL_CASES + S.FUSED_CASES}
    assert met == set(S.INSTANTIATIONS) and len(met) == 36


# ---------------------------------------------------------------------------------------------------------------------
# refusals: the call returns its code and writes nothing
# ---------------------------------------------------------------------------------------------------------------------
_SINGLE = dict(x=1, wt=1, y=1, x_dtype=1, n=2, cin=3, h=18, w=136, cout=16, ld=32, k=3, s=2, pad=1, act=ACT_SILU, dtype=1, pool=0, x_off=0, y_off=0)
_SINGLE_REFUSALS = [
    ("null x", dict(x=0), EINVAL), ("null weights", dict(wt=0), EINVAL), ("null y", dict(y=0), EINVAL),
    ("unknown input type", dict(x_dtype=5), EINVAL), ("uint8 with 4 channels", dict(x_dtype=2, cin=4), EINVAL), ("unknown output type", dict(dtype=7), EINVAL),
    ("cin 0", dict(cin=0), EINVAL), ("cin 5", dict(cin=5), EINVAL), ("cout 6", dict(cout=6), EINVAL), ("cout 0", dict(cout=0), EINVAL),
    ("ldy 36", dict(ld=36), EINVAL), ("y 2 bytes off", dict(y_off=2), EINVAL),
    ("k 0", dict(k=0), EINVAL), ("k 8", dict(k=8), EINVAL), ("stride 0", dict(s=0), EINVAL), ("stride 3", dict(s=3), EINVAL), ("pad -1", dict(pad=-1), EINVAL),
    ("pad = k", dict(pad=3), EINVAL), ("pad > k", dict(k=1, pad=2), EINVAL),
    ("n 0", dict(n=0), EINVAL), ("h 0", dict(h=0), EINVAL), ("w 0", dict(w=0), EINVAL), ("n -1", dict(n=-1), EINVAL),
    ("OH 0", dict(h=2, pad=0), EINVAL), ("OW 0", dict(w=5, k=6, pad=0), EINVAL),
    ("ReLU", dict(act=ACT_RELU), EINVAL), ("bf16 input at an odd address", dict(x_off=1), EINVAL),
    ("pool: odd OH", dict(pool=1, s=1, h=9, w=72), EUNSUPPORTED), ("pool: odd OW", dict(pool=1, s=1, h=10, w=71), EUNSUPPORTED),
    ("pool: f32 output", dict(pool=1, s=1, h=10, w=72, dtype=0), EUNSUPPORTED), ("pool: no activation", dict(pool=1, s=1, h=10, w=72, act=ACT_NONE), EUNSUPPORTED),
    ("pool: stride 2", dict(pool=1), EUNSUPPORTED), ("pool: 48 channels", dict(pool=1, s=1, h=10, w=72, cout=48, ld=64), EUNSUPPORTED),
    ("pool: scalar kernel asked for", dict(pool=1, s=1, h=10, w=72, opts=dict(stem_no_mfma=1)), EUNSUPPORTED),
]


@pytest.mark.parametrize("what,change,code", _SINGLE_REFUSALS, ids=[r[0].replace(" ", "_") for r in _SINGLE_REFUSALS])
@KC.stop_after_fault
def test_stem_refuses_and_writes_nothing(what, change, code):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    a = dict(_SINGLE, **change)
    xd = torch.zeros(4 * 4 * 18 * 136 + 8, dtype=torch.bfloat16, device=DEV)   # room for every shape of the list (never read: the call refuses)
    wd = torch.zeros(7 * 7 * 4 * 64, dtype=torch.float32, device=DEV)
    bd = torch.zeros(64, dtype=torch.float32, device=DEV)
    buf = torch.full((3, 10, 72, 80), NAN, dtype=torch.float32, device=DEV)
    opts = _opts(a.get("opts", {}))
    shape = (a["x_dtype"], a["n"], a["cin"], a["h"], a["w"])
    tail = (a["cout"], a["ld"], a["k"], a["s"], a["pad"], a["act"], a["dtype"])
    xptr = xd.data_ptr() + a["x_off"] if a["x"] else None
    yptr = buf.data_ptr() + 32 + a["y_off"] if a["y"] else None
    if a["x"] and a["wt"] and a["y"] and not a["y_off"]:   # a rule that looks at no pointer: the query answers with the same code
        assert lib.upa_stem_variant(*shape, *tail, a["pool"], C.byref(opts), a["x_off"]) == code, what
    fn = lib.upa_conv2d_stem_nchw_pool2 if a["pool"] else lib.upa_conv2d_stem_nchw
    rc = fn(xptr, *shape, wd.data_ptr() if a["wt"] else None, bd.data_ptr(), yptr, *tail, C.byref(opts), L.current_stream(DEV))
    assert rc == code, (what, rc, lib.upa_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), f"{what}: a refused call wrote to its output"


_FUSED = dict(x=1, w0=1, b0=1, w1=1, b1=1, y=1, n=3, h=36, w=72, k0=3, s0=2, c0=16, ld=48, x_off=0, y_off=0)
_FUSED_REFUSALS = [
    ("null x", dict(x=0)), ("null w0", dict(w0=0)), ("null b0", dict(b0=0)), ("null w1", dict(w1=0)), ("null b1", dict(b1=0)), ("null y", dict(y=0)),
    ("k0 5", dict(k0=5)), ("c0 24", dict(c0=24)), ("c0 32 with k0 6", dict(c0=32, k0=6, ld=80)), ("stride 1 with c0 16", dict(s0=1)), ("stride 3", dict(s0=3)),
    ("stride 0", dict(s0=0)), ("w 76", dict(w=76)), ("h 38", dict(h=38)), ("ldy 52", dict(ld=52)), ("y 2 bytes off", dict(y_off=2)),
    ("n 0", dict(n=0)), ("h 0", dict(h=0)), ("w 0", dict(w=0)), ("n -1", dict(n=-1)),
    ("input 2 bytes into its allocation", dict(x_off=2)), ("input 8 bytes into its allocation", dict(x_off=8)),
]


@pytest.mark.parametrize("what,change", _FUSED_REFUSALS, ids=[r[0].replace(" ", "_") for r in _FUSED_REFUSALS])
@KC.stop_after_fault
def test_fused_stem_refuses_and_writes_nothing(what, change):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    a = dict(_FUSED, **change)
    xd = torch.zeros(4 * 3 * 40 * 80 + 8, dtype=torch.bfloat16, device=DEV)
    w0 = torch.zeros(6 * 6 * 3 * 32, dtype=torch.float32, device=DEV)
    w1 = torch.zeros(9 * 64 * 64, dtype=torch.bfloat16, device=DEV)
    bd = torch.zeros(64, dtype=torch.float32, device=DEV)
    buf = torch.full((4, 20, 40, 96), NAN, dtype=torch.bfloat16, device=DEV)
    opts = _opts({})
    shape = (a["n"], a["h"], a["w"], a["k0"], a["s0"], a["c0"])
    ptrs = [t.data_ptr() if a[k] else None for k, t in (("w0", w0), ("b0", bd), ("w1", w1), ("b1", bd))]
    xptr = xd.data_ptr() + a["x_off"] if a["x"] else None
    yptr = buf.data_ptr() + 16 + a["y_off"] if a["y"] else None
    if all(a[k] for k in ("x", "w0", "b0", "w1", "b1", "y")) and not a["y_off"]:
        assert lib.upa_stem_fused_variant(*shape, a["ld"], C.byref(opts), a["x_off"]) == EINVAL, what
    rc = lib.upa_stem_conv_fused_s(xptr, *shape, *ptrs, yptr, a["ld"], C.byref(opts), L.current_stream(DEV))
    assert rc == EINVAL, (what, rc, lib.upa_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf.float()).all()), f"{what}: a refused call wrote to its output"


@KC.stop_after_fault
def test_fused_model_path_falls_back_to_the_two_layers_on_a_misaligned_input():
    """DetectionModel._stem_fusable looks at the input's address: a bf16 batch that starts 2 bytes into its allocation runs the two layers
    (the stem then stages through VGPRs) instead of raising from the refused fused call - the same result as the aligned batch gives."""
    from tests.hip_utils import DEV, to_cpu_nchw
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    from ultralytics_pro_amd.utils import procedural as P
    m = DetectionModel("yolov8n.yaml")
    P.apply_procedural_weights(m)
    m = m.to(DEV).eval()
    m.set_compute_dtype(torch.bfloat16)
    x = P.uniform("stem_misaligned", (2, 3, 36, 72), 0, 1).to(torch.bfloat16)
    flat = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device=DEV)
    flat[1:1 + x.numel()] = x.flatten().to(DEV)
    xm = flat[1:1 + x.numel()].view(x.shape)
    xa = x.to(DEV)
    assert xm.data_ptr() % 16 == 2 and xm.is_contiguous() and xa.data_ptr() % 16 == 0
    with torch.no_grad():
        place = m._concat_placement()
        assert m._stem_fusable(xa, place) and not m._stem_fusable(xm, place)
        two_m = to_cpu_nchw(m.model[1](m.model[0](xm)))
        two_a = to_cpu_nchw(m.model[1](m.model[0](xa)))
    assert torch.equal(two_m, two_a)
