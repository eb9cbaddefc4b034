"""GPU: the pair-SAD kernel equals the host contract exactly, device and host detection agree, and `cuts=` makes every sequence
entry point treat the shots of a sequence as the separate sequences they are."""
import os

import numpy as np
import pytest
import torch

import shots_cases as sc

pytestmark = pytest.mark.gpu

KINDS = [np.uint8, np.uint16]


def _dev(a: np.ndarray) -> torch.Tensor:
    """Host frames on the device in their dtype (uint16 travels as int16 bits)."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _random(shape, dt, seed):
    rs = np.random.RandomState(seed)
    # uint16: the whole container range, so that a third of the samples lie above 1023 and are clamped
    return rs.randint(0, 256 if dt == np.uint8 else 1536, shape).astype(dt)


# (2,1,4,4): one partial tile; (9,1,23,37): an odd plane, no multiple of 16 bytes, with a byte-wise tail; (9,3,24,40): several
# tiles, three channels; (33,1,36,72): 32 pairs = four whole runs of 8; (12,1,36,72): a whole run and a run of 3
@pytest.mark.parametrize("dt", KINDS)
@pytest.mark.parametrize("shape", [(2, 1, 4, 4), (9, 1, 23, 37), (9, 3, 24, 40), (33, 1, 36, 72), (12, 1, 36, 72)])
def test_kernel_equals_the_host_contract(shape, dt):
    from fcvsr_amd import hip
    from fcvsr_amd.harness.shots import pair_sad_host
    f = _random(shape, dt, seed=shape[0] + shape[3])
    got = hip.frame_pair_sad(_dev(f))
    assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0] - 1,) and got.is_cuda
    assert got.cpu().numpy().tolist() == pair_sad_host(f).tolist()
    # the same bits as int16 (hip.bits16), and from a start that is no multiple of 16 bytes
    if dt == np.uint16:
        assert hip.frame_pair_sad(hip.bits16(_dev(f))).cpu().numpy().tolist() == pair_sad_host(f).tolist()
    assert hip.frame_pair_sad(_dev(f)[1:]).cpu().numpy().tolist() == pair_sad_host(f[1:]).tolist()


@pytest.mark.parametrize("dt", KINDS)
def test_one_frame_gives_an_empty_result_and_bad_input_raises(dt):
    from fcvsr_amd import hip
    one = hip.frame_pair_sad(_dev(_random((1, 1, 8, 8), dt, 0)))
    assert one.dtype == torch.int64 and tuple(one.shape) == (0,)
    with pytest.raises(ValueError):
        hip.frame_pair_sad(torch.zeros(2, 1, 4, 4, device="cuda"))             # float frames
    with pytest.raises(ValueError):
        hip.frame_pair_sad(torch.zeros(2, 4, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError):
        hip.frame_pair_sad(torch.zeros(2, 1, 4, 4, dtype=torch.uint8))


@pytest.mark.parametrize("dt", KINDS)
def test_largest_partial_sums(dt):
    """Frames alternating all-0 and all-peak: every lane, wave and workgroup holds the largest sum it can see at this shape."""
    from fcvsr_amd import hip
    from fcvsr_amd.harness.shots import pair_sad_host
    peak = 255 if dt == np.uint8 else 1023
    f = np.zeros((6, 3, 36, 72), dt)
    f[1::2] = peak
    got = hip.frame_pair_sad(_dev(f)).cpu().numpy().tolist()
    assert got == [peak * 3 * 36 * 72] * 5 == pair_sad_host(f).tolist()
    if dt == np.uint16:                                                        # 65535 reads 1023
        f[1::2] = 65535
        assert hip.frame_pair_sad(_dev(f)).cpu().numpy().tolist() == got


def test_frames_past_two_to_the_31_bytes():
    """Two frames of 2^31 + 1000 bytes: every address of the second frame, and the tile numbers times the tile size, need 64 bits.
    Known answer instead of a host reference: the frames differ in the first 7 and the last 100 samples only."""
    from fcvsr_amd import hip
    n = 2 ** 31 + 1000                                                         # no multiple of 16: a byte-wise tail at the far end
    f = torch.zeros((2, 1, 1, n), dtype=torch.uint8, device="cuda")
    f[1, 0, 0, :7] = 200
    f[1, 0, 0, -100:] = 3
    f[0, 0, 0, -1] = 255
    assert hip.frame_pair_sad(f).cpu().tolist() == [7 * 200 + 99 * 3 + 252]


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_device_and_host_detection_agree(seed):
    from fcvsr_amd.harness.shots import detect_cuts
    cases = [(sc.shots_sequence(seed), sc.CUTS), (sc.shots_sequence(seed, lengths=(12,), pan=3), []), (sc.crossfade_sequence(seed), [])]
    for frames, want in cases:
        for f in (frames, sc.ten_bit(frames)):
            assert detect_cuts(_dev(f)) == detect_cuts(f) == want
    f = sc.shots_sequence(seed)
    for thr in (0.05, 5.0, 18.0):                                              # the same list at other thresholds as well
        assert detect_cuts(_dev(f), threshold=thr) == detect_cuts(f, threshold=thr)


@pytest.fixture(scope="module")
def model():
    from fcvsr_amd.arch.CVSR_freq import GShiftNet_S
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.weights import synthetic_state_dict
    m = GShiftNet_S()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("GShiftNet_S"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    return m


@pytest.fixture(scope="module")
def two_shots():
    """S = A ++ B, 5 and 6 frames of 16 x 20."""
    s = torch.from_numpy(sc.shots_sequence(sc.SEEDS[0], lengths=(5, 6), size=(16, 20)))
    return s, s[:5], s[5:]


@pytest.mark.parametrize("ensemble", [None, "spatial"])
@pytest.mark.parametrize("padding", ["replicate", "reflection"])
def test_cuts_make_the_shots_separate_sequences(model, two_shots, padding, ensemble):
    from fcvsr_amd.harness.infer import super_resolve_sequence
    S, A, B = two_shots
    kw = dict(batch=4, padding=padding, ensemble=ensemble)                     # 11 frames in batches of 4: one straddles the cut
    parts = np.concatenate([super_resolve_sequence(model, A, **kw), super_resolve_sequence(model, B, **kw)], 0)
    got = super_resolve_sequence(model, S, cuts=[5], **kw)
    assert got.shape == (11, 1, 64, 80) and np.array_equal(got, parts)
    plain = super_resolve_sequence(model, S, **kw)
    differs = [i for i in range(11) if not np.array_equal(plain[i], got[i])]
    print(f"padding {padding}, ensemble {ensemble}: frames that differ without cuts: {differs}")
    assert differs and set(differs) <= set(range(2, 8))                        # only the three frames on each side of the cut
    assert np.array_equal(super_resolve_sequence(model, S, cuts=[], **kw), plain)
    if ensemble is None:                                                       # "auto" finds the cut on the device
        assert np.array_equal(super_resolve_sequence(model, S.cuda(), cuts="auto", **kw), got)
        assert np.array_equal(super_resolve_sequence(model, S, cuts=[5], centres=[7, 4], **kw), got[[7, 4]])


def test_evaluate_sequence_auto(model):
    from fcvsr_amd.harness.infer import evaluate_sequence
    lr = torch.from_numpy(sc.shots_sequence(sc.SEEDS[1], lengths=(5, 6)))
    hr = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (11, 1, 4 * sc.H, 4 * sc.W)).astype(np.uint8))
    auto = evaluate_sequence(model, lr, hr, batch=4, cuts="auto", return_frames=True)
    explicit = evaluate_sequence(model, lr, hr, batch=4, cuts=[5], return_frames=True)
    plain = evaluate_sequence(model, lr, hr, batch=4, return_frames=True)
    assert auto.cuts == [5] and explicit.cuts == [5] and plain.cuts is None
    assert np.array_equal(auto.psnr, explicit.psnr) and np.array_equal(auto.ssim, explicit.ssim)
    assert auto.psnr_mean == explicit.psnr_mean and np.array_equal(auto.frames, explicit.frames)
    assert not np.array_equal(plain.frames, explicit.frames)
    none = evaluate_sequence(model, lr, hr, batch=4, cuts="auto", cut_threshold=50.0)      # no pair reaches 50
    assert none.cuts == [] and np.array_equal(none.psnr, plain.psnr)
    # 10-bit frames, with the self-ensemble
    lr10, hr10 = torch.from_numpy(sc.ten_bit(lr.numpy()).view(np.int16)).view(torch.uint16), \
        torch.from_numpy((hr.numpy().astype(np.uint16) * 4).view(np.int16)).view(torch.uint16)
    a10 = evaluate_sequence(model, lr10, hr10, batch=4, cuts="auto", ensemble="spatial")
    e10 = evaluate_sequence(model, lr10, hr10, batch=4, cuts=[5], ensemble="spatial")
    assert a10.cuts == [5] and np.array_equal(a10.psnr, e10.psnr)


def test_super_resolve_yuv420_with_cuts(model, tmp_path):
    from fcvsr_amd.harness.yuv import super_resolve_yuv420, write_yuv420
    H, W = sc.H, sc.W
    y = sc.shots_sequence(sc.SEEDS[2], lengths=(5, 6))[:, 0]
    rs = np.random.RandomState(2)
    u, v = (rs.randint(0, 256, (11, H // 2, W // 2)).astype(np.uint8) for _ in range(2))
    src = str(tmp_path / f"Two_{W}x{H}_11F.yuv")
    write_yuv420(src, y, u, v)

    def run(name, **kw):
        dst = str(tmp_path / name)
        stats = super_resolve_yuv420(model, src, dst, W, H, batch=4, **kw)
        return stats, open(dst, "rb").read()
    s_auto, b_auto = run("auto.yuv", cuts="auto")
    s_cut, b_cut = run("cut.yuv", cuts=[5])
    s_none, b_none = run("none.yuv", cuts=None)
    s_plain, b_plain = run("plain.yuv")
    assert s_auto["cuts"] == [5] and s_cut["cuts"] == [5] and "cuts" not in s_none and "cuts" not in s_plain
    assert b_auto == b_cut and b_none == b_plain and b_cut != b_plain
    assert len(b_cut) == 11 * 16 * H * W * 3 // 2
    # 10 bits: the luma plane is detected on as uint16
    src10 = str(tmp_path / f"Two_{W}x{H}_11F_10bit.yuv")
    write_yuv420(src10, sc.ten_bit(y), u.astype(np.uint16) * 4, v.astype(np.uint16) * 4)
    dst = str(tmp_path / "auto10.yuv")
    stats = super_resolve_yuv420(model, src10, dst, W, H, batch=4, bit_depth=10, cuts="auto")
    auto10 = open(dst, "rb").read()
    assert stats["cuts"] == [5]
    super_resolve_yuv420(model, src10, dst, W, H, batch=4, bit_depth=10, cuts=[5])
    assert open(dst, "rb").read() == auto10


def test_super_resolve_yuv420_rgb_detects_on_the_luma_plane(tmp_path):
    from fcvsr_amd.arch.fcvsr_rgb import FCVSR_SNet
    from fcvsr_amd.arch.schema import state_dict_shapes
    from fcvsr_amd.harness.yuv import super_resolve_yuv420_rgb, write_yuv420
    from fcvsr_amd.weights import synthetic_state_dict
    m = FCVSR_SNet()
    m.load_state_dict(synthetic_state_dict(state_dict_shapes("FCVSR_SNet"), gain=0.5), strict=True)
    m = m.cuda()
    m.precision = "bf16"
    H, W = 16, 20
    y = sc.shots_sequence(sc.SEEDS[0], lengths=(5, 6), size=(H, W))[:, 0]
    u, v = (np.full((11, H // 2, W // 2), 128, np.uint8) for _ in range(2))     # grey chroma: the cut is in the luma alone
    src = str(tmp_path / f"Two_{W}x{H}_11F.yuv")
    write_yuv420(src, y, u, v)
    out = {}
    for name, kw in (("auto", dict(cuts="auto")), ("cut", dict(cuts=[5])), ("plain", {})):
        dst = str(tmp_path / f"{name}.yuv")
        out[name] = (super_resolve_yuv420_rgb(m, src, dst, W, H, batch=4, **kw), open(dst, "rb").read())
    assert out["auto"][0]["cuts"] == [5] and out["cut"][0]["cuts"] == [5] and "cuts" not in out["plain"][0]
    assert out["auto"][1] == out["cut"][1] != out["plain"][1]


def test_streamed_run_with_cuts_equals_the_sequence_path(model):
    from fcvsr_amd.harness.infer import StreamedSuperResolver, super_resolve_sequence
    seqs = [torch.from_numpy(sc.shots_sequence(sc.SEEDS[0], lengths=(5, 6), size=(16, 20))),
            torch.from_numpy(sc.shots_sequence(sc.SEEDS[1], lengths=(3, 2, 4), size=(16, 20))),
            torch.from_numpy(sc.shots_sequence(sc.SEEDS[2], lengths=(6,), size=(16, 20)))]
    cuts = [[5], [3, 5], None]
    for padding in ("replicate", "reflection"):
        got = StreamedSuperResolver(model, batch=4, padding=padding, cuts=cuts).run(seqs)
        for s, (lr, c) in enumerate(zip(seqs, cuts)):
            assert got[s][0] == 0
            assert np.array_equal(got[s][1], super_resolve_sequence(model, lr, batch=4, padding=padding, cuts=c)), (padding, s)
    two = StreamedSuperResolver(model, batch=4, cuts=cuts)                      # two ranks: each its share of the same frames
    whole = StreamedSuperResolver(model, batch=4, cuts=cuts).run(seqs)
    for rank in range(2):
        for s, (first, frames) in two.run(seqs, rank=rank, world=2).items():
            assert np.array_equal(frames, whole[s][1][first:first + len(frames)])
    with pytest.raises(ValueError, match="one list per sequence"):
        StreamedSuperResolver(model, batch=4, cuts=[[5]]).run(seqs)
    with pytest.raises(ValueError, match="strictly increasing"):
        StreamedSuperResolver(model, batch=4, cuts=[[5], [5, 3], None]).run(seqs)
