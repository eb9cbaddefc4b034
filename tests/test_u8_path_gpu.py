"""GPU: uint8 frames in, uint8 SR frames out (`super_resolve_u8`) give exactly the bytes of the float path fed x.float() / 255
(divided on the host) and quantised the harness's way, in every configuration: the dedicated uint8 kernels (16-bit S / full /
RGB twin) and the conversion kernels around the generic layers (exact-f32 mode, 21-channel first layer)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(ctor_name, precision, **attrs):
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    from helpers import get_ctor
    m = get_ctor(ctor_name)()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes(ctor_name), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = precision
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _frames(B, C, H, W, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randint(0, 256, (B, 7, C, H, W)).astype(np.uint8))


def _expected(model, x8, quantise):
    """The float path on x.float() / 255 (host division), then clamp, * 255, optional round, uint8 cast."""
    with torch.no_grad():
        y = model((x8.cpu().float() / 255).cuda())
    y = y.clamp(0, 1) * 255.0
    y = y.round() if quantise == "round" else y
    return y.to(torch.uint8)


def _check(model, x8, quantise):
    got = model.super_resolve_u8(x8.cuda(), quantise)
    ref = _expected(model, x8, quantise)
    assert got.dtype == torch.uint8 and got.shape == ref.shape and got.is_cuda
    mism = int((got != ref).sum())
    assert mism == 0, f"{mism} of {ref.numel()} bytes differ (max {int((got.int() - ref.int()).abs().max())})"
    assert torch.unique(got).numel() > 32          # a real image, not a frame clamped to 0 / 255
    return got


@pytest.mark.parametrize("quantise", ["truncate", "round"])
@pytest.mark.parametrize("precision", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("hw", [(16, 20), (20, 24), (72, 36)])
def test_s_model_u8_equals_float_path(precision, hw, quantise):
    m = _model("GShiftNet_S", precision)
    _check(m, _frames(2, 1, *hw, seed=hw[0] + len(precision)), quantise)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_full_model_bf16_u8_equals_float_path(quantise):
    m = _model("GShiftNet", "bf16")
    _check(m, _frames(1, 1, 20, 24, seed=11), quantise)


@pytest.mark.parametrize("quantise", ["truncate", "round"])
def test_rgb_s_twin_bf16_u8_equals_float_path(quantise):
    m = _model("FCVSR_SNet", "bf16")
    _check(m, _frames(1, 3, 16, 20, seed=12), quantise)


def test_graph_two_streams_batch4_and_no_crosstalk_between_f32_and_u8():
    """hipGraph replay with two streams at B = 4; alternating float and uint8 calls of one shape on one model never replay
    each other's graph (input dtype and quantise mode are part of the key)."""
    m = _model("GShiftNet_S", "bf16", use_graph=True, streams=2)
    xa, xb = _frames(4, 1, 16, 20, seed=21), _frames(4, 1, 16, 20, seed=22)
    ref = {(id(x), q): _expected(m, x, q) for x in (xa, xb) for q in ("truncate", "round")}
    for it in range(2):
        for x in (xa, xb):
            for q in ("truncate", "round"):
                with torch.no_grad():
                    yf = m((x.float() / 255).cuda())            # an f32 call of the same shape in between
                assert yf.dtype == torch.float32
                got = m.super_resolve_u8(x.cuda(), q)
                assert torch.equal(got, ref[(id(x), q)]), (it, q)
    keys = list(m._engine._graphs)
    assert any(torch.uint8 in k for k in keys) and any(torch.float32 in k for k in keys)


def test_non_contiguous_input_view():
    m = _model("GShiftNet_S", "bf16")
    big = _frames(2, 1, 16, 28, seed=31).cuda()
    x = big[:, :, :, :, 4:24]                                  # (2,7,1,16,20), non-contiguous
    assert not x.is_contiguous()
    got = m.super_resolve_u8(x, "round")
    assert torch.equal(got, _expected(m, x.cpu().contiguous(), "round"))


def test_u8_argument_errors_on_the_device():
    m = _model("GShiftNet_S", "bf16")
    x8 = _frames(1, 1, 16, 20, seed=41).cuda()
    with pytest.raises(ValueError, match="multiples of 4"):
        m.super_resolve_u8(x8[..., :18])
    with pytest.raises(ValueError, match="uint8"):
        m.super_resolve_u8(x8.float())
    with pytest.raises(ValueError, match="uint8"):
        m.super_resolve_u8(x8.to(torch.int8))
    with pytest.raises(ValueError, match="quantise"):
        m.super_resolve_u8(x8, "nearest")
    with pytest.raises(ValueError, match="frames"):
        m.super_resolve_u8(x8[:, :5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.super_resolve_u8(x8.cpu())
    with pytest.raises(NotImplementedError):
        _model("GShiftNet_ETC", "bf16").super_resolve_u8(torch.zeros(1, 13, 1, 16, 20, dtype=torch.uint8).cuda())


def test_library_rejects_bad_u8_arguments():
    """The C entry points return FCVSR_E_ARG (-1) instead of launching: wrong dtypes, bad quantise modes, null pointers."""
    import ctypes as C
    from fcvsr_amd import hip
    L = hip.lib()
    tab = hip.u8_table("cuda")
    f = torch.zeros(1, 4, 4, 1, device="cuda")
    b = torch.zeros(1, 16, 16, 1, device="cuda")
    vf, vb = hip.view(f), hip.view(b)
    assert L.fcvsr_bilinear_up4_u8(C.byref(vf), tab.data_ptr(), 1, 4, 4, C.byref(vb), hip.stream_ptr()) == -1   # f32 source
    assert L.fcvsr_quantise_u8(b.data_ptr(), b.numel(), 0, b.data_ptr(), hip.stream_ptr()) == -1             # QUANT_NONE
    assert L.fcvsr_chroma_up4(None, tab.data_ptr(), 1, 2, 2, None, hip.stream_ptr()) == -1
    with pytest.raises(ValueError):
        hip.chroma_up4(torch.zeros(2, 4, 4, device="cuda"))
