"""-m gpu: every kernel family `upa_conv2d_bias_act` can dispatch to (conv_path() in csrc/conv.hip), called through the C ABI on
channel slices of wider buffers and compared with the float64 reference and the per-element bound of tests/conv_ref.py.

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py
(input ldx = cin + 2 E
with 7.0 - NaN in `poison` - beside the slice, output ldy = cout + 3 E with four spare rows, residual ldr = cout + E, bias padded with 7.0);
weights hold values the storage type holds exactly, and every case first asserts the kernel family through `upa_conv_variant`.
The bound is conv_ref.conv_bound; the `print`s give the worst error / bound of each case (pytest -s)."""

import ctypes as C

import pytest
import torch

from tests import conv_ref as CR
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

SPARE = 4
PAD = 7.0
NONE, SILU, RELU = CR.ACT_NONE, CR.ACT_SILU, CR.ACT_RELU
BF16, F32 = torch.bfloat16, torch.float32
ALL = ("uniform", "poison", "saturated", "impulse", "impulse2")
UPA_EINVAL, UPA_EUNSUPPORTED = -1, -2
PATH_BITS = {"ws": 20, "pipe": 21, "c1": 22, "big": 23, "ws3": 24, "p8": 26}


def _path(variant):
    assert variant >= 0, f"upa_conv_variant failed: {variant}"
    for name, bit in PATH_BITS.items():
        if (variant >> bit) & 1:
            return name
    return "igemm"


class _Problem:
    """One convolution laid out as the file's conventions say: device buffers, their pitches and the view pointers."""

    def __init__(self, x, w, bias, res, k, stride, pad, dtype, poison=False):
        DEV, L, lib, _ = KC.env()
        self.n, self.cin, self.h, self.w = x.shape
        self.cout, self.k, self.stride, self.pad, self.dtype = w.shape[0], k, stride, pad, dtype
        self.es = torch.empty(0, dtype=dtype).element_size()
        E = self.E = 16 // self.es
        self.oh, self.ow = (self.h + 2 * pad - k) // stride + 1, (self.w + 2 * pad - k) // stride + 1
        self.code = L.dtype_code(dtype)
        self.ldx, self.ldy, self.ldr = self.cin + 2 * E, self.cout + 3 * E, self.cout + E
        self.xbuf = KC.slice_buf(x.permute(0, 2, 3, 1), dtype, E, fill=float("nan") if poison else PAD)
        assert self.xbuf.shape[-1] == self.ldx
        self.x_ptr = self.xbuf.data_ptr() + E * self.es
        wc = w.contiguous().float()
        assert torch.equal(wc.to(dtype).float(), wc), "weights not representable: packing would round"
        packed = torch.empty(lib.upa_conv_packed_weight_bytes(self.cout, self.cin, k, self.code), dtype=torch.uint8)
        L.check(lib.upa_pack_conv_weight(wc.data_ptr(), self.cout, self.cin, k, self.code, packed.data_ptr()), "pack")
        self.wbuf = packed.to(DEV)
        self.bbuf = None
        if bias is not None:
            bb = torch.full((-(-self.cout // 16) * 16,), PAD, dtype=torch.float32)
            bb[:self.cout] = bias
            self.bbuf = bb.to(DEV)
        self.rbuf = None
        if res is not None:
            rb = torch.full((self.n * self.oh * self.ow, self.ldr), PAD, dtype=dtype)
            rb[:, :self.cout] = res.permute(0, 2, 3, 1).reshape(-1, self.cout).to(dtype)
            self.rbuf = rb.to(DEV)

    @property
    def rows(self):
        return self.n * self.oh * self.ow

    def new_out(self):
        return KC.out_buf((self.rows,), self.ldy, self.dtype, SPARE)

    def y_ptr(self, ybuf):
        return ybuf.data_ptr() + self.E * self.es

    def variant(self, opts):
        lib = KC.env()[2]
        return lib.upa_conv_variant(self.n, self.h, self.w, self.cin, self.cout, self.k, self.stride, self.pad, self.code, C.byref(opts))

    def run(self, ybuf, act, opts):
        _, _, lib, st = KC.env()
        return lib.upa_conv2d_bias_act(self.x_ptr, self.n, self.h, self.w, self.cin, self.ldx, self.wbuf.data_ptr(),
                                       self.bbuf.data_ptr() if self.bbuf is not None else None, self.y_ptr(ybuf), self.cout, self.ldy,
                                       self.rbuf.data_ptr() if self.rbuf is not None else None, self.ldr if self.rbuf is not None else 0,
                                       self.k, self.stride, self.pad, act, self.code, C.byref(opts), st)

    def payload(self, bufs, what):
        """Both runs identical in every bit, everything outside the slice still NaN, payload finite -> NCHW float64 of the first run."""
        out = KC.payload_of_two(bufs, self.rows, self.cout, what, offset=self.E)
        return out.reshape(self.n, self.oh, self.ow, self.cout).permute(0, 3, 1, 2).double()


def _opts(**kw):
    from ultralytics_pro_amd import _lib as L
    return L.Opts(**kw)


def _run_case(n, cin, h, w, cout, k, stride, pad, act, dtype, opts, family, seed, with_bias=True, with_res=False, want=None, what=""):
    """One family of one case: layout, path assertion, two runs, layout checks.  Returns (y, v, S, ref, bound) as NCHW float64."""
    DEV, L, lib, _ = KC.env()
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x, wt, bias, res = CR.conv_family(family, n, cin, h, w, cout, k, dtype, seed, with_bias, with_res, (oh, ow))
    P = _Problem(x, wt, bias, res, k, stride, pad, dtype, poison=family == "poison")
    var = P.variant(opts)
    if want is not None:
        want(var)
    ys = [P.new_out() for _ in range(2)]
    for y in ys:
        L.check(P.run(y, act, opts), what)
    torch.cuda.synchronize()
    y = P.payload(ys, what)
    v, S, ref = CR.conv_ref(x, wt, bias, res, k, stride, pad, act)
    return y, v, S, ref, CR.conv_bound(v, S, ref, cin * k * k, act, dtype)


def _check_families(n, cin, h, w, cout, k, stride, pad, act, dtype, opts, report, families=ALL, with_bias=True, with_res=False, want=None, seed=0):
    for i, family in enumerate(families):
        what = (f"{'bf16' if dtype == BF16 else 'f32'} {family} n{n} {cin}->{cout} {h}x{w} k{k}s{stride}p{pad} act{act}"
                f"{'' if with_bias else ' nobias'}{' res' if with_res else ''}")
        y, v, S, ref, bound = _run_case(n, cin, h, w, cout, k, stride, pad, act, dtype, opts, family, seed * 16 + i, with_bias, with_res, want, what)
        if family == "saturated":
            assert float(v.max()) > 60 and float(v.min()) < -60, what
        KC.check_bound(y, ref, bound, what, report)


def _want(path, tile=None, ckt=None, low=None):
    def f(var):
        assert _path(var) == path, f"variant {var:#x}: path {_path(var)}, wanted {path}"
        if tile is not None:
            assert var & 0xFFFF == tile, f"variant {var:#x}: tile {var & 0xFFFF:#x}, wanted {tile:#x}"
        if ckt is not None:
            assert (var >> 16) & 0xF == ckt, f"variant {var:#x}: k-tiles per chunk {(var >> 16) & 0xF}, wanted {ckt}"
        if low is not None:
            assert low(var & 0xFFFF), f"variant {var:#x}"
    return f


# =====================================================================================================================
# 1. the generic kernel: conv_igemm_kernel<T, WM, WN, MTW, NTW, CKT>
# =====================================================================================================================
def _igemm_opts(dtype, **kw):
    if dtype == BF16:  # every other family switched off
        return _opts(conv_big=1, conv_ws3=1, conv_p8=1, no_pipe=1, no_1x1=1, no_ws=1, **kw)
    return _opts(no_ws=1, **kw)


def _igemm_tile(cout, M):
    """dispatch_conv's choice (WM << 12 | WN << 8 | MTW << 4 | NTW)."""
    ntn = -(-cout // 16)
    if ntn <= 3:
        return 0x4120 | ntn
    if ntn == 5:
        return 0x2243 if M >= 128 * 1024 else 0x2223
    if ntn % 4 == 0:
        return 0x2242 if (M >= 128 * 1024 or ntn == 4) else 0x2222
    return 0x4122 if ntn % 2 == 0 else 0x4121


# cin, cout, (k, stride, pad), act, bias, residual
IGEMM_BF16 = [
    (8, 8, (1, 1, 0), SILU, True, False),      # NTn 1, a quarter k-tile, pointwise form (pixels flattened)
    (24, 24, (2, 1, 1), RELU, True, True),     # NTn 2, even kernel: output one larger than the input
    (40, 48, (3, 1, 1), NONE, False, False),   # NTn 3, two k-tiles (the second a quarter full), no bias
    (72, 64, (3, 2, 1), SILU, True, True),     # NTn 4, three k-tiles in three chunks
    (24, 80, (3, 1, 0), RELU, True, False),    # NTn 5 as 2 x 3 tiles with a zero sixth; valid convolution
    (40, 72, (3, 1, 2), SILU, False, True),    # NTn 5 with half of the fifth tile real; pad 2 > k / 2
    (8, 96, (4, 2, 1), NONE, True, False),     # NTn 6
    (24, 112, (5, 1, 2), SILU, True, True),    # NTn 7
    (72, 128, (7, 2, 3), RELU, True, False),   # NTn 8 on the 64-pixel tile
    (72, 24, (5, 1, 2), RELU, False, True),    # odd tap count over three chunks: the carried weight buffer
]
IGEMM_F32 = [
    (4, 4, (1, 1, 0), SILU, True, False),
    (20, 12, (2, 1, 1), RELU, True, True),
    (4, 20, (3, 1, 1), NONE, False, False),
    (20, 36, (3, 2, 1), SILU, True, True),
    (20, 64, (3, 1, 0), RELU, True, False),
    (36, 80, (3, 1, 2), SILU, False, True),    # three chunks: the per-chunk partial sums folded into a running total
    (4, 96, (4, 2, 1), NONE, True, False),
    (20, 112, (5, 1, 2), SILU, True, True),
    (4, 128, (7, 2, 3), RELU, True, False),
    (36, 12, (5, 1, 2), RELU, False, True),
]


def _ids(cases):
    return [f"c{c[0]}-{c[1]}_k{c[2][0]}s{c[2][1]}p{c[2][2]}_a{c[3]}{'' if c[4] else '_nob'}{'_res' if c[5] else ''}" for c in cases]


def _igemm_case(case, dtype, idx):
    cin, cout, (k, s, p), act, bias, res = case
    n, h, w = 2, 13, 11
    M = n * ((h + 2 * p - k) // s + 1) * ((w + 2 * p - k) // s + 1)
    report = []
    _check_families(n, cin, h, w, cout, k, s, p, act, dtype, _igemm_opts(dtype), report, with_bias=bias, with_res=res,
           want=_want("igemm", tile=_igemm_tile(cout, M)), seed=100 + idx)
    # measured on MI355X (worst error / bound over the ten cases): bf16 0.996 (the output rounding itself: half an ulp at the foot of a
    # binade), f32 0.204 (k 5, 20 channels in, impulse family)
    KC.print_report(report, f"igemm {dtype} {case}")


@pytest.mark.parametrize("case", IGEMM_BF16, ids=_ids(IGEMM_BF16))
@KC.stop_after_fault
def test_igemm_bf16(case):
    """The generic bf16 kernel with every other family switched off, 2 x 13 x 11 maps: one case per n-tile count of dispatch_conv,
    every (k, stride, pad) the issue lists, cin 8 / 24 / 40 / 72 (partial k-tiles), cout 8 / 24 / 72 (partial n-tiles), all three
    activations, no bias, residual on its own pitch."""
    _igemm_case(case, BF16, IGEMM_BF16.index(case))


@pytest.mark.parametrize("case", IGEMM_F32, ids=_ids(IGEMM_F32))
@KC.stop_after_fault
def test_igemm_f32(case):
    """The same for the f32 parity mode (two-phase LDS epilogue, IEEE divide SiLU): cin 4 / 20 / 36, cout 4 / 12 / 20 / 36."""
    _igemm_case(case, F32, 50 + IGEMM_F32.index(case))


@pytest.mark.parametrize("ckt", [1, 2, 4])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_igemm_chunk_override(dtype, ckt):
    """upa_opts.conv_ckt = 1 | 2 | 4 on a four-k-tile shape (bf16 128, f32 64 channels in): 4, 2 and 1 chunks of LDS staging."""
    report = []
    cin = 128 if dtype == BF16 else 64
    _check_families(2, cin, 13, 11, 32, 3, 1, 1, SILU, dtype, _igemm_opts(dtype, conv_ckt=ckt), report, families=("uniform", "poison", "impulse"),
           with_res=True, want=_want("igemm", tile=0x4122, ckt=ckt), seed=200 + ckt)
    # measured on MI355X: bf16 0.975, f32 0.103
    KC.print_report(report, f"igemm {dtype} ckt {ckt}")


@pytest.mark.parametrize("cout,tile", [(80, 0x2243), (128, 0x2242)], ids=["c80_2243", "c128_2242"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_igemm_large_map_tiles(dtype, cout, tile):
    """The two M >= 128 * 1024 tiles: 2 x 256 x 256 pixels, 8 (f32: 4) channels in."""
    report = []
    _check_families(2, 8 if dtype == BF16 else 4, 256, 256, cout, 3, 1, 1, SILU, dtype, _igemm_opts(dtype), report, families=("poison", "impulse"),
           want=_want("igemm", tile=tile), seed=300 + cout)
    # measured on MI355X: bf16 0.994, f32 0.115
    KC.print_report(report, f"igemm {dtype} large map cout {cout}")


# =====================================================================================================================
# 2. the weights-stationary generic kernel: conv_ws_kernel<T, WM, WN, MTW, NTW, KTT>
# =====================================================================================================================
def _ws_launches(ktt, ntn):
    """launch_ws's admission: weight slab + two halo buffers + 1 KiB must fit LDS twice (perCU >= 2).  256-pixel tiles (16 x 16, halo
    18 x 18), for NTn 4 also 128-pixel ones (8 x 16, halo 10 x 18); a pixel of the halo takes 64 KTT bytes."""
    def lds(bm, ntb):
        halo = -(-((bm // 16 + 2) * 18 * ktt * 4) // 64) * 64 * 16
        return 9 * ktt * ntb * 1024 + 2 * halo + 1024
    return any(lds(bm, ntn) <= 80 * 1024 for bm in ((256, 128) if ntn == 4 else (256,)))


@pytest.mark.parametrize("cout", [16, 32, 64])
@pytest.mark.parametrize("ktt", [1, 2, 4])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_ws_kernel(dtype, ktt, cout):
    """Default options, k 3 s 1, 1 x 256 x 256 (M = 64 * 1024, the kernel's threshold), KTT = 1 | 2 | 4 k-tiles of input channels
    (the first two partly filled), 1 / 2 / 4 n-tiles.  Reading launch_ws: the perCU >= 2 rule admits KTT = 1 only - two halo buffers
    of a 256-pixel tile at KTT = 2 are 81 KiB, and at 128 pixels the 64-channel weight slab no longer fits beside them - so the
    KTT = 2 and 4 instantiations exist but are never launched; _ws_launches restates the rule and the case asserts that
    upa_conv_variant agrees, so the day the rule changes these cases cover the kernel.  Either way the result is held to the bound,
    and where the weights-stationary kernel runs, it and the tile-per-workgroup kernel (no_ws = 1) are within each other's bounds
    (|a - b| <= 2 bound)."""
    E = 8 if dtype == BF16 else 4
    cin = {1: 3 * E, 2: 5 * E, 4: 16 * E}[ktt]
    expect_ws = _ws_launches(ktt, cout // 16)
    assert expect_ws == (ktt == 1)
    # cout 64 with 128 channels in would go to conv_big by the size rule; every other combination reaches the generic dispatch
    opts = _opts(conv_big=1) if dtype == BF16 else _opts()
    report = []
    for i, family in enumerate(("poison", "impulse")):
        what = f"ws {dtype} ktt {ktt} cout {cout} {family}"
        args = (1, cin, 256, 256, cout, 3, 1, 1, SILU, dtype)
        y, v, S, ref, bound = _run_case(*args, opts, family, 400 + i, True, True, _want("ws" if expect_ws else "igemm"), what)
        # measured on MI355X: conv_ws_kernel (KTT 1) bf16 0.996, f32 0.191; the KTT 2 / 4 shapes on conv_igemm_kernel bf16 0.989, f32 0.384
        KC.check_bound(y, ref, bound, what, report)
        if expect_ws:
            y2 = _run_case(*args, opts.replace(no_ws=1), family, 400 + i, True, True, _want("igemm"), what + " no_ws")[0]
            KC.check_bound(y, y2, 2 * bound, f"{what}: ws against igemm (2 bound)")
    KC.print_report(report, f"ws {dtype} ktt {ktt} cout {cout}")


# =====================================================================================================================
# 3. conv_ws3
# =====================================================================================================================
WS3_CASES = [  # cin, (h, w), act, residual
    (8, (9, 5), SILU, False), (24, (17, 19), RELU, True), (48, (33, 16), NONE, False), (64, (9, 5), RELU, False),
    (64, (17, 19), SILU, True), (8, (33, 16), NONE, True), (24, (9, 5), SILU, True), (48, (17, 19), RELU, False),
]


@pytest.mark.parametrize("case", WS3_CASES, ids=[f"c{c[0]}_{c[1][0]}x{c[1][1]}_a{c[2]}{'_res' if c[3] else ''}" for c in WS3_CASES])
@KC.stop_after_fault
def test_conv_ws3(case):
    """conv_ws3_kernel (conv_ws3 = 2): one and two k-tiles, both partly filled (cin 8 / 24 / 48), maps narrower than a tile, with ragged
    tiles on both axes and with several tiles per workgroup; all three activations, with and without the residual."""
    cin, (h, w), act, res = case
    report = []
    _check_families(2, cin, h, w, 64, 3, 1, 1, act, BF16, _opts(conv_ws3=2), report, with_res=res, with_bias=cin != 48, want=_want("ws3"),
           seed=500 + WS3_CASES.index(case))
    # measured on MI355X: 0.995
    KC.print_report(report, f"ws3 {case}")


# =====================================================================================================================
# 4. conv_p8
# =====================================================================================================================
P8_CASES = [  # cin, cout, (h, w), act, residual
    (64, 128, (4, 4), RELU, False), (128, 128, (7, 9), NONE, True), (64, 256, (20, 20), SILU, False), (128, 256, (7, 9), SILU, True),
    (128, 128, (20, 20), RELU, True),
]


@pytest.mark.parametrize("case", P8_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2][0]}x{c[2][1]}_a{c[3]}{'_res' if c[4] else ''}" for c in P8_CASES])
@KC.stop_after_fault
def test_conv_p8(case):
    """conv_p8_kernel (conv_p8 = 2): one and two 64-channel chunks, one and two 128-channel columns, the smallest map it takes, a
    ragged one and one with several tiles; ReLU, none and SiLU, the residual."""
    cin, cout, (h, w), act, res = case
    report = []
    _check_families(2, cin, h, w, cout, 3, 1, 1, act, BF16, _opts(conv_p8=2), report, with_res=res, with_bias=(h, w) != (7, 9) or cin == 128 and cout == 256,
           want=_want("p8"), seed=600 + P8_CASES.index(case))
    # measured on MI355X: 0.993
    KC.print_report(report, f"p8 {case}")


# =====================================================================================================================
# 5. conv_big
# =====================================================================================================================
BIG_CASES = [  # cin, cout, (k, stride), bm, (h, w), act, residual
    (8, 64, (1, 1), 0, (9, 13), SILU, False),
    (24, 72, (2, 1), 128, (21, 19), RELU, True),
    (72, 80, (3, 1), 256, (21, 19), NONE, False),
    (96, 88, (3, 2), 128, (9, 13), SILU, True),
    (24, 128, (3, 1), 256, (21, 19), RELU, False),
    (72, 64, (3, 1), 512, (21, 19), SILU, True),
    (8, 80, (3, 1), 512, (9, 13), RELU, False),
    (96, 128, (1, 1), 256, (21, 19), NONE, True),
    (72, 72, (3, 2), 256, (21, 19), NONE, True),
    (96, 64, (2, 1), 0, (9, 13), RELU, False),
    (24, 88, (1, 1), 128, (9, 13), SILU, False),
    (8, 128, (3, 2), 0, (21, 19), SILU, False),
]


@pytest.mark.parametrize("case", BIG_CASES, ids=[f"c{c[0]}-{c[1]}_k{c[2][0]}s{c[2][1]}_bm{c[3]}_{c[4][0]}x{c[4][1]}_a{c[5]}{'_res' if c[6] else ''}"
                                                 for c in BIG_CASES])
@KC.stop_after_fault
def test_conv_big(case):
    """conv_big (conv_big = 2, ws3 and p8 off): every (k, stride) it has, 64- / 80- / 96- / 128-channel columns with cout 72 and 88
    filling the last n-tile half, cin from a quarter k-tile to three, workgroups of 128, 256 and - where the form has it - 512 pixels
    on ragged maps; ReLU, the residual on its own pitch.  A 1x1 case with a residual is among them (conv_big comes before
    conv1x1_stream in the order of preference)."""
    cin, cout, (k, s), bm, (h, w), act, res = case
    report = []

    def low(v):  # n-tiles per workgroup << 4 | pixels per workgroup / 128
        return bm == 0 or (v & 0xF) == bm >> 7
    _check_families(2, cin, h, w, cout, k, s, k // 2, act, BF16, _opts(conv_big=2, conv_ws3=1, conv_p8=1, conv_big_bm=bm), report, with_res=res,
           with_bias=cin != 24, want=_want("big", low=low), seed=700 + BIG_CASES.index(case))
    # measured on MI355X: 0.993
    KC.print_report(report, f"big {case}")


# =====================================================================================================================
# 6. / 7. conv3x3_pipe and conv3x3_c16
# =====================================================================================================================
PIPE_CASES = [  # cin, cout, (h, w), act, residual, pipe_wgs
    (8, 16, (8, 16), SILU, False, 0), (24, 48, (24, 32), NONE, True, 2), (80, 80, (24, 32), SILU, True, 2), (128, 16, (8, 16), NONE, False, 0),
    (128, 80, (24, 32), SILU, False, 2), (24, 16, (24, 32), SILU, True, 2), (80, 48, (8, 16), NONE, False, 0),
]


@pytest.mark.parametrize("case", PIPE_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2][0]}x{c[2][1]}_a{c[3]}{'_res' if c[4] else ''}_wgs{c[5]}" for c in PIPE_CASES])
@KC.stop_after_fault
def test_conv_pipe(case):
    """conv3x3_pipe_kernel<NTW 1 | 2 | 4> (pipe_all = 1, pipe_min_tiles = 1): one to four k-tiles with the last partly filled, output
    channels in launches of 64 / 32 / 16, one tile per image and 3 x 2; pipe_wgs = 2 makes every wave walk several tiles."""
    cin, cout, (h, w), act, res, wgs = case
    report = []
    _check_families(2, cin, h, w, cout, 3, 1, 1, act, BF16, _opts(pipe_all=1, pipe_min_tiles=1, pipe_wgs=wgs), report, with_res=res,
           with_bias=cin != 80, want=_want("pipe", low=lambda v: not v & 0x100), seed=800 + PIPE_CASES.index(case))
    # measured on MI355X: 0.992
    KC.print_report(report, f"pipe {case}")


C16_CASES = [  # cout, (h, w), act, residual, c16_wgs
    (16, (24, 32), SILU, True, 2), (16, (8, 16), NONE, False, 0), (32, (24, 32), SILU, False, 2), (32, (8, 16), NONE, False, 0),
    (16, (24, 32), NONE, True, 0), (32, (24, 32), SILU, True, 2),
]


@pytest.mark.parametrize("case", C16_CASES, ids=[f"c16-{c[0]}_{c[1][0]}x{c[1][1]}_a{c[2]}{'_res' if c[3] else ''}_wgs{c[4]}" for c in C16_CASES])
@KC.stop_after_fault
def test_conv_c16(case):
    """conv3x3_c16_kernel: 16 -> 16 and, with pipe_all, 16 -> 32; residual; c16_wgs = 2.  16 -> 32 with a residual has no c16 form:
    upa_conv_variant (which sees no residual) names c16, the call itself runs conv3x3_pipe_kernel<2> - the result is what counts."""
    cout, (h, w), act, res, wgs = case
    report = []
    _check_families(2, 16, h, w, cout, 3, 1, 1, act, BF16, _opts(pipe_all=1, pipe_min_tiles=1, c16_wgs=wgs, pipe_wgs=wgs), report, with_res=res,
           want=_want("pipe", low=lambda v: bool(v & 0x100)), seed=900 + C16_CASES.index(case))
    # measured on MI355X: 0.994
    KC.print_report(report, f"c16 {case}")


@KC.stop_after_fault
def test_pipe_refuses_relu():
    """conv3x3_pipe has no ReLU form: upa_conv_pipe_eligible must send it elsewhere (the launcher would run it as `none`).  The variant
    query passes no activation, so the result is the evidence: negative outputs would appear."""
    report = []
    _check_families(2, 24, 8, 16, 32, 3, 1, 1, RELU, BF16, _opts(pipe_all=1, pipe_min_tiles=1), report, families=("uniform", "saturated"), seed=950)
    # measured on MI355X: 0.957
    KC.print_report(report, "pipe relu")


# =====================================================================================================================
# 8. conv1x1_stream
# =====================================================================================================================
C1_CASES = [  # cin, cout, act, opts - overrides chosen as test_hip_ops.py's C1_CASES chooses them
    (8, 8, SILU, {}),                                          # a quarter k-tile, half an n-tile
    (24, 24, NONE, {"c1_mt": 2, "c1_waves": 8}),               # pair store with the upper half masked
    (96, 80, SILU, {"c1_mt": 4, "c1_wgs": 2}),                 # NTW 5 (odd tail store), three k-tiles, many rounds per wave
    (24, 136, NONE, {"c1_mt": 2, "c1_wgs": 1}),                # 9 n-tiles: a second workgroup row with half an n-tile
    (96, 192, SILU, {"c1_waves": 4}),                          # 12 n-tiles: second row half masked
    (8, 192, SILU, {"c1_mt": 1, "c1_waves": 4, "c1_wgs": 2}),
    (96, 8, NONE, {"c1_mt": 4, "c1_wgs": 3}),
]


@pytest.mark.parametrize("case", C1_CASES, ids=[f"c{c[0]}-{c[1]}_a{c[2]}{'_' + '_'.join(str(v) for v in c[3].values()) if c[3] else ''}" for c in C1_CASES])
@KC.stop_after_fault
def test_conv1x1_stream(case):
    """conv1x1_stream_kernel (default options): 3 x 7 x 9 = 189 pixels (ragged last pixel tile), partial k-tiles, masked / odd / split
    n-tiles, every (MT, waves) override."""
    cin, cout, act, kw = case
    report = []

    def low(v):  # waves << 8 | MT << 4 | NTW
        return ("c1_mt" not in kw or (v >> 4) & 0xF == kw["c1_mt"]) and ("c1_waves" not in kw or (v >> 8) & 0xF == kw["c1_waves"])
    _check_families(3, cin, 7, 9, cout, 1, 1, 0, act, BF16, _opts(**kw), report, with_bias=cout != 136, want=_want("c1", low=low), seed=1000 + C1_CASES.index(case))
    # measured on MI355X: 0.992
    KC.print_report(report, f"c1 {case}")


@KC.stop_after_fault
def test_1x1_with_residual_leaves_the_stream_kernel():
    """conv1x1_stream has no residual input: upa_conv1x1_eligible refuses s.ldr != 0.  upa_conv_variant sees no residual and names the
    stream kernel for this shape; the call with a residual must come back with the residual added, under default options and with
    conv_big forced as well (where the variant must not carry bit 22)."""
    report = []
    _check_families(3, 24, 7, 9, 80, 1, 1, 0, SILU, BF16, _opts(), report, with_res=True, want=_want("c1"), seed=1100)
    _check_families(3, 24, 7, 9, 80, 1, 1, 0, SILU, BF16, _opts(conv_big=2), report, with_res=True, want=_want("big"), seed=1101)
    # measured on MI355X: 0.993
    KC.print_report(report, "1x1 residual")


# =====================================================================================================================
# 9. refusals and the group entry
# =====================================================================================================================
def _refusal_problem(dtype, cin=None, k=3, stride=1, pad=1, h=6, w=5, cout=None, res=True):
    E = 8 if dtype == BF16 else 4
    cin, cout = cin or 2 * E, cout or 2 * E
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x, wt, bias, r = CR.conv_family("uniform", 2, cin, h, w, cout, k, dtype, 1200, True, res, (oh, ow))
    return _Problem(x, wt, bias, r, k, stride, pad, dtype), (x, wt, bias, r)


def _raw_call(P, ybuf, opts, **over):
    """upa_conv2d_bias_act on problem P with single arguments replaced."""
    _, _, lib, st = KC.env()
    a = dict(x=P.x_ptr, n=P.n, h=P.h, w=P.w, cin=P.cin, ldx=P.ldx, wp=P.wbuf.data_ptr(), bias=P.bbuf.data_ptr(), y=P.y_ptr(ybuf), cout=P.cout,
             ldy=P.ldy, res=P.rbuf.data_ptr() if P.rbuf is not None else None, ldr=P.ldr if P.rbuf is not None else 0, k=P.k, stride=P.stride,
             pad=P.pad, act=SILU)
    a.update(over)
    return lib.upa_conv2d_bias_act(a["x"], a["n"], a["h"], a["w"], a["cin"], a["ldx"], a["wp"], a["bias"], a["y"], a["cout"], a["ldy"], a["res"],
                                   a["ldr"], a["k"], a["stride"], a["pad"], a["act"], P.code, C.byref(opts), st)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_refusals_leave_the_output_untouched(dtype):
    """What conv_check and the pointer checks reject comes back as UPA_EINVAL with nothing launched: the NaN output stays NaN.  The
    arguments are otherwise those of a valid call on a buffer large enough for every variation tried."""
    P, _ = _refusal_problem(dtype)
    E, es = P.E, P.es
    ybuf = P.new_out()
    opts = _opts()
    bad = {
        "cin % E": dict(cin=P.cin - 1),
        "ldy % E": dict(ldy=P.ldy - 1),
        "ldx % E": dict(ldx=P.ldx - 1),
        "pad >= k": dict(pad=3),
        "k = 8": dict(k=8, pad=4),
        "stride = 3": dict(stride=3),
        "misaligned x": dict(x=P.x_ptr + es),
        "misaligned y": dict(y=P.y_ptr(ybuf) + es),
        "misaligned residual": dict(res=P.rbuf.data_ptr() + es),
        "residual with ldr = 0": dict(ldr=0),
    }
    for name, over in bad.items():
        assert _raw_call(P, ybuf, opts, **over) == UPA_EINVAL, name
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf.float()).all()), "a refused call wrote to its output"
    assert _raw_call(P, ybuf, opts) == 0  # ... and the unvaried call is a valid one
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ybuf.float()[:P.rows, E:E + P.cout]).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_k7_stride2_wide_input_fits_or_is_refused_cleanly(dtype):
    """k 7, stride 2, 512 channels in: the largest halo the generic kernel can be asked for.  Reading launch_conv_ckt, k > 3 always
    stages one k-tile per chunk, so its 21 x 37-pixel halo is 49 KiB whatever cin is and the UPA_EUNSUPPORTED return ("tile does not fit
    LDS") cannot be reached through upa_conv2d_bias_act today.  The contract is checked both ways: a refusal must leave the NaN output
    untouched, a run must meet the bound (eight chunks of k-tiles, 49 taps each)."""
    cin = 512 if dtype == BF16 else 256
    n, h, w, cout = 2, 35, 33, 16  # 18 x 17 outputs: 16-wide tiles, the full 21 x 37 halo
    x, wt, bias, _ = CR.conv_family("uniform", n, cin, h, w, cout, 7, dtype, 1300)
    P = _Problem(x, wt, bias, None, 7, 2, 3, dtype, poison=True)
    DEV, L, lib, _ = KC.env()
    opts = _igemm_opts(dtype)
    ys = [P.new_out() for _ in range(2)]
    rcs = [P.run(y, RELU, opts) for y in ys]
    torch.cuda.synchronize()
    assert rcs[0] == rcs[1] and rcs[0] in (0, UPA_EUNSUPPORTED), rcs
    if rcs[0] == UPA_EUNSUPPORTED:
        assert all(bool(torch.isnan(y.float()).all()) for y in ys)
        return
    y = P.payload(ys, "k7 s2")
    v, S, ref = CR.conv_ref(x, wt, bias, None, 7, 2, 3, RELU)
    # measured on MI355X: both dtypes run (rc 0); bf16 0.064, f32 below 0.001 (K = 25088 / 12544: the accumulation term dominates the bound)
    what = f"k7 s2 cin {cin} {dtype}"
    print(f"{what}: worst error / bound = {KC.check_bound(y, ref, CR.conv_bound(v, S, ref, cin * 49, RELU, dtype), what):.3f}")


def _group_check(specs, k, stride, pad, act, dtype, opts, what):
    """specs: (n, cin, h, w, cout) per problem.  upa_conv2d_bias_act_group on strided views against one upa_conv2d_bias_act per problem
    under the same opts: bit-identical, sentinels untouched; the single calls are held to the bound."""
    DEV, L, lib, st = KC.env()
    probs, singles, grouped, refs = [], [], [], []
    for i, (n, cin, h, w, cout) in enumerate(specs):
        x, wt, bias, _ = CR.conv_family("poison", n, cin, h, w, cout, k, dtype, 1400 + i)
        P = _Problem(x, wt, bias, None, k, stride, pad, dtype, poison=True)
        probs.append(P)
        refs.append((CR.conv_ref(x, wt, bias, None, k, stride, pad, act), cin))
        singles.append(P.new_out())
        grouped.append(P.new_out())
        L.check(P.run(singles[-1], act, opts), what)
    arr = (L.ConvProblem * len(probs))()
    for q, P, y in zip(arr, probs, grouped):
        q.x, q.n, q.h, q.w, q.cin, q.ldx = P.x_ptr, P.n, P.h, P.w, P.cin, P.ldx
        q.w_packed, q.bias, q.y, q.cout, q.ldy, q.residual, q.ldr = P.wbuf.data_ptr(), P.bbuf.data_ptr(), P.y_ptr(y), P.cout, P.ldy, None, 0
    L.check(lib.upa_conv2d_bias_act_group(arr, len(probs), k, stride, pad, act, L.dtype_code(dtype), C.byref(opts), st), what)
    torch.cuda.synchronize()
    for P, s, g, ((v, S, ref), cin) in zip(probs, singles, grouped, refs):
        y = P.payload((s, g), what)  # (asserts group == single in every bit, sentinels included)
        KC.check_bound(y, ref, CR.conv_bound(v, S, ref, cin * k * k, act, dtype), what)


@KC.stop_after_fault
def test_group_three_problems_on_strided_views():
    """Three problems of different kernels' shapes (generic, conv_ws3 by force, generic) through the group entry."""
    _group_check([(2, 24, 13, 11, 24), (2, 64, 9, 16, 64), (1, 8, 5, 7, 80)], 3, 1, 1, SILU, BF16, _opts(conv_ws3=2), "group of three")
    _group_check([(2, 4, 13, 11, 12), (2, 20, 9, 16, 64), (1, 4, 5, 7, 80)], 3, 1, 1, RELU, F32, _opts(), "group of three f32")


@pytest.mark.parametrize("no_group", [0, 1])
@KC.stop_after_fault
def test_group_conv_big_pairs(no_group):
    """Two problems sharing a conv_big 128-pixel instantiation (64 + 64 channels out), and a 64- next to an 80-channel problem (the
    five-tile instantiation takes both): one grid under no_group = 0, one launch per problem under no_group = 1; identical either way."""
    opts = _opts(conv_big=2, conv_ws3=1, conv_p8=1, conv_big_bm=128, no_group=no_group)
    _group_check([(2, 72, 21, 19, 64), (2, 24, 9, 13, 64)], 3, 1, 1, SILU, BF16, opts, f"conv_big pair 64 + 64 no_group {no_group}")
    _group_check([(2, 24, 21, 19, 64), (2, 72, 9, 13, 80)], 3, 1, 1, RELU, BF16, opts, f"conv_big pair 64 + 80 no_group {no_group}")
    _group_check([(2, 64, 21, 19, 64), (2, 64, 9, 13, 64)], 3, 1, 1, SILU, BF16, opts.replace(conv_big_bm=0),
                 f"conv_big pair, workgroup size by rule, no_group {no_group}")
