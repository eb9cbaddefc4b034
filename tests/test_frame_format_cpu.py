"""CPU: the dtype of a tensor selects the entry point and the sample table of the frame-boundary kernels together (`hip._ENTRIES`,
`hip._entry`, `hip.sample_table` and the wrappers `Engine._forward` calls).  `hip.lib` and `hip.stream_ptr` are stand-ins that record
calls and the table cache holds host tensors, so no device is touched."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float32, torch.uint8, torch.uint16)
INT_SYMBOL = re.compile(r"_u8$|_u16$|_u8_to_f32$|_u16_to_f32$")
COLOUR = {"fcvsr_yuv420_to_rgb_u16", "fcvsr_rgb_to_yuv420_u16"}       # dispatched in harness.colour, not one of hip's families


def _sample_bytes(symbol):
    """The size of the samples an entry point reads (its first kernels) or writes (its last ones), from its name."""
    return 1 if re.search(r"_u8$|_u8_to_", symbol) else 2 if re.search(r"_u16$|_u16_to_", symbol) else 4


def _table_position(symbol):
    """The index of the ``tab`` parameter in the header's declaration of `symbol`, None if it has none."""
    hdr = open(os.path.join(ROOT, "include", "fcvsr_hip.h")).read()
    params = re.search(r"\bint " + symbol + r"\s*\(([^;]*)\)\s*;", hdr).group(1).split(",")
    at = [i for i, p in enumerate(params) if re.search(r"\btab$", p.strip())]
    assert len(at) <= 1
    return at[0] if at else None


class _Recorder:
    """Stands in for the loaded library: every fcvsr_* call is recorded and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fcvsr_"):
            raise AttributeError(name)

        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    from fcvsr_amd import hip
    r = _Recorder()
    monkeypatch.setattr(hip, "lib", lambda: r)
    monkeypatch.setattr(hip, "stream_ptr", lambda: 0)
    r.tables = {torch.uint8: torch.zeros(256), torch.uint16: torch.zeros(1024)}
    for dt, t in r.tables.items():
        monkeypatch.setitem(hip._SAMPLE_TABLES, (dt, "cpu"), t)
    return r


def _ptr_of(arg):
    """The address an argument carries: a raw pointer, or the `ptr` of a View passed by reference."""
    return arg._obj.ptr if hasattr(arg, "_obj") else arg


def _check_call(rec, symbol, selector, selector_at):
    """The one recorded call is `symbol` with the argument count of its signature, tensor `selector` (whose dtype chose it) at
    argument `selector_at`, samples of the size the symbol reads, and the table of that dtype exactly where the header has one."""
    from fcvsr_amd import hip
    assert len(rec.calls) == 1, rec.calls
    name, args = rec.calls.pop()
    assert name == symbol
    assert len(args) == len(hip.SIGNATURES[name])
    assert _ptr_of(args[selector_at]) == selector.data_ptr()
    if hasattr(args[selector_at], "_obj"):
        assert args[selector_at]._obj.dtype == hip._DT[selector.dtype]
    assert selector.element_size() == _sample_bytes(name)               # uint8 frames never reach a kernel that reads 2-byte samples
    at = _table_position(name)
    tabs = {t.data_ptr() for t in rec.tables.values()}
    if at is None:
        assert not tabs & {a for a in args if isinstance(a, int)}
    else:
        tab = rec.tables[selector.dtype]
        assert tab.numel() == (256 if selector.dtype == torch.uint8 else 1024) and args[at] == tab.data_ptr()
        assert not tabs & {a for i, a in enumerate(args) if isinstance(a, int) and i != at}
    return args


def test_every_entry_name_is_a_declared_symbol_and_the_families_cover_the_integer_symbols():
    from fcvsr_amd import hip
    produced = {s for fam in hip._ENTRIES.values() for s in fam.values()}
    assert produced <= set(hip.SIGNATURES), produced - set(hip.SIGNATURES)
    integer = {s for s in hip.SIGNATURES if INT_SYMBOL.search(s)} - COLOUR
    # the f32 form of fcvsr_<name>_u8 / _u16 is fcvsr_<name> where the header has one; chroma_up4 and frame_metrics spell their uint8
    # form that way
    plain = {re.sub(r"_u8$|_u16$", "", s) for s in integer} & set(hip.SIGNATURES)
    assert produced == integer | plain, produced ^ (integer | plain)
    for fam in hip._ENTRIES.values():
        assert set(fam) <= set(DTYPES) and {torch.uint8, torch.uint16} <= set(fam)
        for dt, s in fam.items():
            if dt != torch.float32 and s not in ("fcvsr_chroma_up4", "fcvsr_frame_metrics"):
                assert _sample_bytes(s) == torch.empty(0, dtype=dt).element_size(), s
    assert set(hip._INT_FORMATS) == {torch.uint8, torch.uint16}
    assert [hip._INT_FORMATS[d][:2] for d in (torch.uint8, torch.uint16)] == [(hip.U8, 255), (hip.U16, hip.PEAK10)]


def test_the_named_tables_are_the_cached_object_of_sample_table(rec):
    from fcvsr_amd import hip
    assert hip.u8_table("cpu") is hip.sample_table(torch.uint8, "cpu") is rec.tables[torch.uint8]
    assert hip.u16_table(torch.device("cpu")) is hip.sample_table(torch.uint16, "cpu") is rec.tables[torch.uint16]
    assert torch.equal(hip._INT_FORMATS[torch.uint8][2](), torch.arange(256, dtype=torch.uint8).float() / 255)
    assert torch.equal(hip._INT_FORMATS[torch.uint16][2](), torch.arange(1024, dtype=torch.int32).float() / 1023)
    with pytest.raises(KeyError):
        hip.sample_table(torch.float32, "cpu")


def _suffix(dt):
    return {torch.float32: "", torch.uint8: "_u8", torch.uint16: "_u16"}[dt]


@pytest.mark.parametrize("Cimg", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "u8", "u16"])
def test_first_kernels_follow_the_dtype_of_the_window(rec, dt, Cimg):
    from fcvsr_amd import hip
    B, T, H, W, n = 1, 7, 4, 4, 64
    x = torch.zeros((B, T, Cimg, H, W), dtype=dt)
    if dt == torch.float32:
        with pytest.raises(KeyError):                                   # f32 frames need no conversion: there is no such entry
            hip.samples_to_f32(x, torch.empty_like(x))
        assert not rec.calls
    else:
        xf = torch.empty(x.shape)
        hip.samples_to_f32(x, xf)
        args = _check_call(rec, f"fcvsr_{_suffix(dt)[1:]}_to_f32", x, 0)
        assert args[2] == x.numel() and args[3] == xf.data_ptr()
    xin = x.view(B, T * Cimg, H, W).permute(0, 2, 3, 1)
    dsts = [torch.empty((B, H, W, n), dtype=torch.bfloat16) for _ in range(7)]
    wf, bf = torch.empty(64, 7 * n, dtype=torch.bfloat16), torch.empty(7 * n)
    hip.feat_extract(xin, B, H, W, wf, bf, dsts, n, hip.BF16)
    args = _check_call(rec, "fcvsr_feat_extract" + _suffix(dt), xin, 0)
    k = 1 if dt == torch.float32 else 2
    assert args[k:k + 3] == (B, H, W) and args[k + 5] == 7 and list(args[k + 6]) == [d.data_ptr() for d in dsts]
    assert list(args[k + 7]) == [n] * 7 and list(args[k + 8]) == [0] * 7 and args[k + 9] == hip.BF16
    centre = x[:, T // 2].permute(0, 2, 3, 1)
    base = torch.empty((B, Cimg, 4 * H, 4 * W)).permute(0, 2, 3, 1)
    hip.bilinear_up4(centre, base)
    args = _check_call(rec, "fcvsr_bilinear_up4" + _suffix(dt), centre, 0)
    assert args[k:k + 3] == (B, H, W) and _ptr_of(args[k + 3]) == base.data_ptr()


@pytest.mark.parametrize("Cimg", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "u8", "u16"])
def test_last_kernels_follow_the_dtype_of_the_result(rec, dt, Cimg):
    from fcvsr_amd import hip
    B, T, H, W, n = 1, 7, 4, 4, 64
    integer = dt != torch.float32
    quant = hip.QUANT_ROUND if integer else None
    x = torch.zeros((B, T, Cimg, H, W), dtype=dt)
    centre = x[:, T // 2].permute(0, 2, 3, 1)
    out = torch.zeros((B, Cimg, 4 * H, 4 * W), dtype=dt).permute(0, 2, 3, 1)
    base = torch.empty((B, Cimg, 4 * H, 4 * W)).permute(0, 2, 3, 1) if integer else out      # an f32 result accumulates in place
    u1, u2 = torch.empty((B, 2 * H, 2 * W, n), dtype=torch.bfloat16), torch.empty((B, 4 * H, 4 * W, n), dtype=torch.bfloat16)
    w2, b2, slope, wl, bl = torch.empty(256, 64), torch.empty(256), torch.empty(1), torch.empty(32, 64), torch.empty(Cimg)
    fused = (u1, w2, b2, slope, wl, bl, B, 2 * H, 2 * W, out)

    for kw in ({}, dict(base=base, centre=centre)):                     # exactly one of the two
        with pytest.raises(ValueError):
            hip.tail_fused(*fused, quant=quant, **kw)
    assert not rec.calls

    hip.tail_fused(*fused, base=base, quant=quant)
    args = _check_call(rec, "fcvsr_tail_fused" + _suffix(dt), out, 10 if integer else 9)
    assert args[6:9] == (B, 2 * H, 2 * W) and _ptr_of(args[9]) == base.data_ptr() and _ptr_of(args[0]) == u1.data_ptr()
    assert args[-2] == quant if integer else len(args) == 11

    hip.tail_fused(*fused, centre=centre, quant=quant)
    args = _check_call(rec, "fcvsr_tail_fused_base" + _suffix(dt), out, 11 if integer else 10)
    assert _ptr_of(args[6]) == centre.data_ptr() and args[6]._obj.dtype == hip._DT[dt]      # the centre frame is read in the same format
    assert args[8 if integer else 7:][:3] == (B, 2 * H, 2 * W)
    assert args[-2] == quant if integer else len(args) == 12

    hip.conv_last(u2, wl, bl, B, 4 * H, 4 * W, Cimg, base, out, quant)
    args = _check_call(rec, "fcvsr_conv_last" + _suffix(dt), out, 8 if integer else 7)
    assert args[3:7] == (B, 4 * H, 4 * W, Cimg) and _ptr_of(args[7]) == base.data_ptr()
    assert args[-2] == quant if integer else len(args) == 9

    res = torch.empty((B, Cimg, 4 * H, 4 * W))
    dense = torch.zeros(res.shape, dtype=dt)
    if integer:
        hip.quantise(res, dense, quant)
        args = _check_call(rec, "fcvsr_quantise" + _suffix(dt), dense, 3)
        assert args[:3] == (res.data_ptr(), res.numel(), quant)
    else:
        with pytest.raises(KeyError):                                   # an f32 result is not quantised: there is no such entry
            hip.quantise(res, dense, quant)
        assert not rec.calls
