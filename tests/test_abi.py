"""CPU (-m "not gpu"): the C-ABI library builds, loads and exports every symbol include/upa.h declares; the ctypes
prototype table covers the header; the product path refuses to run without a GPU (no CPU fallback)."""

import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def _header_functions():
    text = (ROOT / "include" / "upa.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(upa_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from ultralytics_pro_amd import _lib
    if not _lib.LIB_PATH.is_file():
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/upa.h but not exported"
    assert set(names) == set(_lib.PROTOTYPES), "ctypes prototype table and include/upa.h disagree"
    assert _lib.lib().upa_version() >= 1


def test_host_side_weight_packing_layout():
    """upa_pack_conv_weight is host code: check the documented fragment order without a GPU."""
    from ultralytics_pro_amd import _lib as L
    cout, cin, k = 20, 24, 3
    w = torch.arange(cout * cin * k * k, dtype=torch.float32).reshape(cout, cin, k, k)
    for code, E, esz in ((L.UPA_F32, 4, 4), (L.UPA_BF16, 8, 2)):
        nbytes = L.lib().upa_conv_packed_weight_bytes(cout, cin, k, code)
        ktch = 4 * E
        ktt, ntn = -(-cin // ktch), -(-cout // 16)
        assert nbytes == k * k * ktt * ntn * 1024
        host = torch.zeros(nbytes, dtype=torch.uint8)
        L.check(L.lib().upa_pack_conv_weight(w.data_ptr(), cout, cin, k, code, host.data_ptr()))
        vals = host.view(torch.float32) if code == L.UPA_F32 else host.view(torch.bfloat16).float()
        vals = vals.reshape(k * k, ktt, ntn, 4, 16, E)
        wref = w.to(torch.bfloat16).float() if code == L.UPA_BF16 else w
        for (tap, kt, nt, g, r, j) in [(0, 0, 0, 0, 0, 0), (4, 0, 1, 2, 3, 1), (8, ktt - 1, 0, 1, 15, E - 1)]:
            co, ci = nt * 16 + r, kt * ktch + g * E + j
            exp = float(wref[co, ci, tap // k, tap % k]) if (co < cout and ci < cin) else 0.0
            assert float(vals[tap, kt, nt, g, r, j]) == exp


def test_dispatch_options_travel_with_the_call_and_the_library_reads_no_environment(monkeypatch):
    """Round-2 review item 4: include/upa.h promises no global state.  The dispatch query (host logic only, no launch) must follow
    the caller's `upa_opts`, two different option sets must not influence each other, and UPA_* environment variables must be
    ignored by the library (they were process-global switches in rounds 1-2)."""
    import ctypes as C
    import subprocess
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    assert lib.upa_opts_size() == C.sizeof(L.Opts)
    q = (32, 40, 40, 128, 64, 3, 1, 1, L.UPA_BF16)  # yolov8n Detect cv2[1][0]: 128 -> 64 3x3 at 40x40, bs 32
    big = lambda v: (v >> 23) & 1  # noqa: E731
    default = lib.upa_conv_variant(*q, None)
    assert big(default)
    never, always = L.Opts(conv_big=1), L.Opts(conv_big=2)
    assert not big(lib.upa_conv_variant(*q, C.pointer(never)))
    assert lib.upa_conv_variant(*q, None) == default                      # the previous call left no mode behind
    small = (1, 16, 16, 128, 64, 3, 1, 1, L.UPA_BF16)                     # too few pixels for the size rule ...
    assert not big(lib.upa_conv_variant(*small, None)) and big(lib.upa_conv_variant(*small, C.pointer(always)))  # ... forced
    v128 = lib.upa_conv_variant(*q, C.pointer(L.Opts(conv_big_bm=128)))
    v256 = lib.upa_conv_variant(*q, C.pointer(L.Opts(conv_big_bm=256)))
    assert (v128 & 15, v256 & 15) == (1, 2)                                # pixels per workgroup / 128
    short = L.Opts(conv_big=1)
    short.size = 8                                                         # an older caller whose struct ends after conv_big
    assert not big(lib.upa_conv_variant(*q, C.pointer(short)))
    monkeypatch.setenv("UPA_CONV_BIG", "0")                                # the round-2 switch for "never": must be ignored now
    monkeypatch.setenv("UPA_CONV_BIG_BM", "128")
    assert lib.upa_conv_variant(*q, None) == default
    src = (ROOT / "ultralytics_pro_amd" / "csrc")
    hits = subprocess.run(["grep", "-ln", "getenv", *[str(f) for f in sorted(src.glob("*.hip")) + sorted(src.glob("*.h"))]],
                          capture_output=True, text=True).stdout.split()
    assert hits == [], f"getenv in the library sources: {hits}"
    ws3 = lambda v: (v >> 24) & 1  # noqa: E731
    q64 = (32, 40, 40, 64, 64, 3, 1, 1, L.UPA_BF16)                        # 64 -> 64 3x3: the persistent kernel by default ...
    assert ws3(lib.upa_conv_variant(*q64, None)) and big(lib.upa_conv_variant(*q64, C.pointer(L.Opts(conv_ws3=1))))  # ... conv_big on request
    assert L.Opts.from_env({"UPA_NO_PAIR": "0", "UPA_C1_MT": "4", "UPA_CONV_FORCE": "4,1,2,4"}).pair == 2  # tool-side mapping only


def test_conv_p8_dispatch_rule_is_host_logic():
    """The round-4 dispatch rule of the two-group phased kernel (csrc/conv_p8.hip: one-round layers of 256-pixel x 128-channel tiles with
    Cin >= 256) is pure host logic behind `upa_conv_variant`: the layers it was measured on pick it, their neighbours stay on conv_big,
    `upa_opts.conv_p8` = 1 / 2 switch it off / force it, and bit 25 (the removed conv_mm kernel) is never chosen."""
    import ctypes as C
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    p8 = lambda v: (v >> 26) & 1   # noqa: E731
    big = lambda v: (v >> 23) & 1  # noqa: E731
    mm = lambda v: (v >> 25) & 1   # noqa: E731
    one_round = [(16, 40, 40, 512, 256), (16, 20, 20, 512, 1024), (16, 40, 40, 768, 256), (32, 20, 20, 256, 512), (32, 40, 40, 256, 128)]
    others = [(16, 40, 40, 256, 512), (16, 80, 80, 256, 128), (16, 80, 80, 128, 256), (16, 20, 20, 1024, 512), (32, 40, 40, 128, 128)]
    for n, h, w, c1, c2 in one_round:
        v = lib.upa_conv_variant(n, h, w, c1, c2, 3, 1, 1, L.UPA_BF16, None)
        assert p8(v) and not mm(v), (n, h, w, c1, c2, hex(v))
        assert big(lib.upa_conv_variant(n, h, w, c1, c2, 3, 1, 1, L.UPA_BF16, C.pointer(L.Opts(conv_p8=1))))
    for n, h, w, c1, c2 in others:
        v = lib.upa_conv_variant(n, h, w, c1, c2, 3, 1, 1, L.UPA_BF16, None)
        assert big(v) and not p8(v) and not mm(v), (n, h, w, c1, c2, hex(v))
        assert p8(lib.upa_conv_variant(n, h, w, c1, c2, 3, 1, 1, L.UPA_BF16, C.pointer(L.Opts(conv_p8=2))))
    assert not p8(lib.upa_conv_variant(16, 40, 40, 512, 256, 3, 2, 1, L.UPA_BF16, C.pointer(L.Opts(conv_p8=2))))  # stride 2: never


# upa_conv_variant of every distinct conv shape the five bench.py workloads issue (bf16 at 640 x 640: yolov8n / yolov8s / yolov3-tiny /
# yolov5-BoT3 at batch 32, yolov3-rtdetr at batch 16; the stem's 3-channel convs run elsewhere; plus yolov8n's stacked 144-channel first
# Detect conv), recorded before the conv dispatch was folded into one selector: (n, h, w, cin, cout, k, stride, pad, (library defaults,
# the in-flight runner's upa_opts of engine/pipeline.py, tests/conftest.py's TEST_OPTS))
CONV_VARIANTS = [
    (16, 20, 20, 512, 256, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (16, 20, 20, 512, 1024, 3, 1, 1, (0x4000082, 0x4000082, 0x4000082)),
    (16, 20, 20, 1024, 256, 1, 1, 0, (0x800041, 0x800041, 0x800041)),
    (16, 20, 20, 1024, 512, 1, 1, 0, (0x800041, 0x800041, 0x800041)),
    (16, 20, 20, 1024, 512, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (16, 40, 40, 256, 128, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (16, 40, 40, 256, 512, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (16, 40, 40, 512, 256, 1, 1, 0, (0x400818, 0x800081, 0x400818)),
    (16, 40, 40, 512, 256, 3, 1, 1, (0x4000082, 0x4000082, 0x4000082)),
    (16, 40, 40, 512, 1024, 3, 2, 1, (0x800081, 0x800081, 0x800081)),
    (16, 40, 40, 768, 256, 3, 1, 1, (0x4000082, 0x4000082, 0x4000082)),
    (16, 80, 80, 128, 256, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (16, 80, 80, 256, 128, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (16, 80, 80, 256, 256, 1, 1, 0, (0x400828, 0x800082, 0x400828)),
    (16, 80, 80, 256, 512, 3, 2, 1, (0x800082, 0x800082, 0x800082)),
    (16, 80, 80, 384, 128, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (16, 160, 160, 64, 128, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (16, 160, 160, 128, 64, 3, 1, 1, (0x800042, 0x800042, 0x800042)),
    (16, 160, 160, 128, 256, 3, 2, 1, (0x800082, 0x800082, 0x800082)),
    (16, 320, 320, 32, 64, 3, 1, 1, (0x200004, 0x800042, 0x200004)),
    (16, 320, 320, 64, 32, 3, 1, 1, (0x200002, 0x200002, 0x200002)),
    (16, 320, 320, 64, 128, 3, 2, 1, (0x800082, 0x800082, 0x800082)),
    (16, 640, 640, 32, 64, 3, 2, 1, (0x12242, 0x800042, 0x12242)),
    (32, 20, 20, 64, 64, 1, 1, 0, (0x400814, 0x800041, 0x400814)),
    (32, 20, 20, 64, 64, 3, 1, 1, (0x1000044, 0x800041, 0x1000044)),
    (32, 20, 20, 80, 80, 1, 1, 0, (0x400815, 0x800061, 0x400815)),
    (32, 20, 20, 80, 80, 3, 1, 1, (0x800051, 0x800051, 0x800051)),
    (32, 20, 20, 128, 80, 1, 1, 0, (0x400815, 0x800061, 0x400815)),
    (32, 20, 20, 128, 128, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (32, 20, 20, 128, 128, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 256, 64, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 256, 80, 1, 1, 0, (0x400815, 0x800061, 0x400815)),
    (32, 20, 20, 256, 80, 3, 1, 1, (0x800051, 0x800051, 0x800051)),
    (32, 20, 20, 256, 128, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (32, 20, 20, 256, 256, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (32, 20, 20, 256, 256, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 256, 512, 3, 1, 1, (0x4000082, 0x4000082, 0x4000082)),
    (32, 20, 20, 384, 256, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (32, 20, 20, 512, 64, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 512, 128, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 512, 256, 1, 1, 0, (0x400818, 0x800041, 0x400818)),
    (32, 20, 20, 512, 256, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 512, 512, 1, 1, 0, (0x400818, 0x800081, 0x400818)),
    (32, 20, 20, 512, 1024, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 20, 20, 768, 512, 1, 1, 0, (0x800081, 0x800081, 0x800081)),
    (32, 20, 20, 1024, 256, 1, 1, 0, (0x800041, 0x800041, 0x800041)),
    (32, 20, 20, 1024, 512, 1, 1, 0, (0x800081, 0x800081, 0x800081)),
    (32, 40, 40, 64, 64, 1, 1, 0, (0x400824, 0x800041, 0x400824)),
    (32, 40, 40, 64, 64, 3, 1, 1, (0x1000044, 0x800041, 0x1000044)),
    (32, 40, 40, 80, 80, 1, 1, 0, (0x400825, 0x800061, 0x400825)),
    (32, 40, 40, 80, 80, 3, 1, 1, (0x800051, 0x800051, 0x800051)),
    (32, 40, 40, 128, 64, 1, 1, 0, (0x400824, 0x800041, 0x400824)),
    (32, 40, 40, 128, 64, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 40, 40, 128, 80, 1, 1, 0, (0x400825, 0x800061, 0x400825)),
    (32, 40, 40, 128, 80, 3, 1, 1, (0x800051, 0x800051, 0x800051)),
    (32, 40, 40, 128, 128, 1, 1, 0, (0x400828, 0x800081, 0x400828)),
    (32, 40, 40, 128, 128, 3, 1, 1, (0x800081, 0x800081, 0x800081)),
    (32, 40, 40, 128, 128, 3, 2, 1, (0x800041, 0x800041, 0x800041)),
    (32, 40, 40, 128, 256, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 40, 40, 128, 256, 3, 2, 1, (0x800041, 0x800041, 0x800041)),
    (32, 40, 40, 192, 128, 1, 1, 0, (0x400828, 0x800081, 0x400828)),
    (32, 40, 40, 256, 64, 1, 1, 0, (0x400824, 0x800041, 0x400824)),
    (32, 40, 40, 256, 64, 3, 1, 1, (0x800041, 0x800041, 0x800041)),
    (32, 40, 40, 256, 80, 1, 1, 0, (0x400825, 0x800061, 0x400825)),
    (32, 40, 40, 256, 128, 1, 1, 0, (0x400828, 0x800081, 0x400828)),
    (32, 40, 40, 256, 128, 3, 1, 1, (0x4000082, 0x4000082, 0x4000082)),
    (32, 40, 40, 256, 256, 1, 1, 0, (0x400828, 0x800082, 0x400828)),
    (32, 40, 40, 256, 256, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 40, 40, 256, 256, 3, 2, 1, (0x800041, 0x800041, 0x800041)),
    (32, 40, 40, 256, 512, 3, 2, 1, (0x800081, 0x800081, 0x800081)),
    (32, 40, 40, 384, 128, 1, 1, 0, (0x400828, 0x800081, 0x400828)),
    (32, 40, 40, 384, 256, 1, 1, 0, (0x400828, 0x800082, 0x400828)),
    (32, 40, 40, 384, 256, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 40, 40, 512, 256, 1, 1, 0, (0x400818, 0x800082, 0x400818)),
    (32, 40, 40, 768, 256, 1, 1, 0, (0x800082, 0x800082, 0x800082)),
    (32, 80, 80, 32, 32, 1, 1, 0, (0x400842, 0x400842, 0x400842)),
    (32, 80, 80, 32, 32, 3, 1, 1, (0x200002, 0x200002, 0x200002)),
    (32, 80, 80, 64, 32, 1, 1, 0, (0x400842, 0x400842, 0x400842)),
    (32, 80, 80, 64, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 80, 80, 64, 64, 3, 1, 1, (0x1000044, 0x800042, 0x1000044)),
    (32, 80, 80, 64, 64, 3, 2, 1, (0x22242, 0x800041, 0x22242)),
    (32, 80, 80, 64, 80, 3, 1, 1, (0x800052, 0x800052, 0x800052)),
    (32, 80, 80, 64, 128, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 80, 80, 64, 128, 3, 2, 1, (0x800081, 0x800081, 0x800081)),
    (32, 80, 80, 80, 80, 1, 1, 0, (0x400845, 0x800062, 0x400845)),
    (32, 80, 80, 80, 80, 3, 1, 1, (0x800052, 0x800052, 0x800052)),
    (32, 80, 80, 96, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 80, 80, 128, 32, 1, 1, 0, (0x400842, 0x400842, 0x400842)),
    (32, 80, 80, 128, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 80, 80, 128, 64, 3, 1, 1, (0x800042, 0x800042, 0x800042)),
    (32, 80, 80, 128, 80, 1, 1, 0, (0x400845, 0x800062, 0x400845)),
    (32, 80, 80, 128, 128, 1, 1, 0, (0x400848, 0x800082, 0x400848)),
    (32, 80, 80, 128, 128, 3, 1, 1, (0x800082, 0x800082, 0x800082)),
    (32, 80, 80, 128, 128, 3, 2, 1, (0x800081, 0x800081, 0x800081)),
    (32, 80, 80, 128, 256, 3, 2, 1, (0x800082, 0x800082, 0x800082)),
    (32, 80, 80, 192, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 80, 80, 192, 128, 1, 1, 0, (0x400848, 0x800082, 0x400848)),
    (32, 80, 80, 256, 128, 1, 1, 0, (0x400828, 0x800082, 0x400828)),
    (32, 80, 80, 384, 128, 1, 1, 0, (0x400828, 0x800082, 0x400828)),
    (32, 160, 160, 16, 16, 1, 1, 0, (0x400841, 0x400841, 0x400841)),
    (32, 160, 160, 16, 16, 3, 1, 1, (0x200101, 0x200101, 0x200101)),
    (32, 160, 160, 32, 16, 1, 1, 0, (0x400841, 0x400841, 0x400841)),
    (32, 160, 160, 32, 32, 1, 1, 0, (0x400842, 0x400842, 0x400842)),
    (32, 160, 160, 32, 32, 3, 1, 1, (0x200002, 0x200002, 0x200002)),
    (32, 160, 160, 32, 64, 3, 1, 1, (0x200004, 0x800042, 0x200004)),
    (32, 160, 160, 32, 64, 3, 2, 1, (0x12242, 0x800042, 0x12242)),
    (32, 160, 160, 48, 32, 1, 1, 0, (0x400842, 0x400842, 0x400842)),
    (32, 160, 160, 64, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 160, 160, 64, 128, 3, 2, 1, (0x800082, 0x800082, 0x800082)),
    (32, 160, 160, 96, 64, 1, 1, 0, (0x400844, 0x800042, 0x400844)),
    (32, 320, 320, 16, 32, 3, 1, 1, (0x200102, 0x200102, 0x200102)),
    (32, 320, 320, 16, 32, 3, 2, 1, (0x14122, 0x14122, 0x14122)),
    (32, 320, 320, 32, 64, 3, 2, 1, (0x12242, 0x800042, 0x12242)),
    (32, 80, 80, 64, 144, 3, 1, 1, (0x800092, 0x800092, 0x800092)),
]


def test_conv_dispatch_matches_the_recorded_table():
    """Every bench workload's conv shape picks the same kernel family and instantiation (the variant bits bench.py / tools decode) under the
    three option sets callers use."""
    import ctypes as C
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    optsets = [None, L.Opts(c2f=4, conv_ws3=1, c2f_stream_rows=-1, detect_stream=2, conv_big=2),
               L.Opts(pipe_min_tiles=1, pipe_all=1, pair=2, c2f64_max_px=-1)]
    bad = []
    for *shape, expected in CONV_VARIANTS:
        got = tuple(lib.upa_conv_variant(*shape, L.UPA_BF16, None if o is None else C.pointer(o)) for o in optsets)
        if got != expected:
            bad.append((shape, [hex(v) for v in expected], [hex(v) for v in got]))
    assert not bad, bad


def test_product_builds_on_cpu_but_refuses_to_run_there():
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov8n.yaml")
    assert sum(p.numel() for p in m.parameters()) == 3157200
    with pytest.raises(UpaError):
        m(torch.zeros(1, 3, 64, 64))


def test_stem_dispatch_query_names_what_every_stem_case_runs():
    """`upa_stem_variant` / `upa_stem_fused_variant` are host logic (the one selector the launchers go through): without a GPU they must answer
    every case of tests/stem_ref.py with the family, instantiation, staging form, waves and workgroup count the case states, follow the
    input's alignment (a bf16 input off its 16 bytes: VGPR staging for the plain stem, UPA_EINVAL for the fused pair) and refuse with the
    launch's own codes."""
    import ctypes as C
    from tests import stem_ref as S
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    code = {"f32": L.UPA_F32, "bf16": L.UPA_BF16, "u8": L.UPA_U8_BGR_HWC}
    for c in S.SINGLE_CASES + S.POOL_CASES:
        ld = 16 + c["cout"] + (-c["cout"] % 8)
        v = lib.upa_stem_variant(code[c["fmt"]], c["n"], c["cin"], c["h"], c["w"], c["cout"], ld, c["k"], c["s"], c["pad"], c["act"], code[c["out"]],
                                 c["pool"], C.pointer(L.Opts(**c["opts"])), 2 if c["misalign"] else 0)
        assert v >= 0 and S.decode_variant(v) == c["expect"], (c["id"], v)
    for c in S.FUSED_CASES:
        q = (c["n"], c["h"], c["w"], c["k0"], c["s0"], c["c0"], 2 * c["c0"] + 16, C.pointer(L.Opts(**c["opts"])))
        v = lib.upa_stem_fused_variant(*q, 0)
        assert v >= 0 and S.decode_variant(v) == c["expect"], (c["id"], v)
        assert lib.upa_stem_fused_variant(*q, 2) == L.UPA_EINVAL
    q = (L.UPA_BF16, 2, 3, 18, 136, 16, 32, 3, 2, 1, L.ACT_SILU, L.UPA_BF16, 0, None)
    assert [S.decode_variant(lib.upa_stem_variant(*q, a))["staging"] for a in (0, 2, 8, 16)] == [S.DMA, S.VGPR, S.VGPR, S.DMA]
    assert lib.upa_stem_variant(*q, 1) == L.UPA_EINVAL                                      # a bf16 input at an odd address
    assert lib.upa_stem_variant(*q[:9], 3, *q[10:], 0) == L.UPA_EINVAL                      # pad >= k
    assert lib.upa_stem_variant(*q[:3], 1, *q[4:9], 0, *q[10:], 0) == L.UPA_EINVAL          # h 1, k 3, pad 0: no output row
    assert lib.upa_stem_variant(*q[:12], 1, None, 0) == L.UPA_EUNSUPPORTED                  # pool on a stride-2 stem
