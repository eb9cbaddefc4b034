"""GPU: every instantiation of the FFT kernels (csrc/fft.hip) against torch.fft in float64 on the CPU, with the path the call took.

fcvsr_rfft2 / fcvsr_irfft2 / fcvsr_irfft2_bands choose between per-length two-stage kernels (twelve lengths N = R1 * R2, one template
instantiation per length, source dtype, direction and mask) and the multi-stage plan kernels (any length; a 16-byte `vec` path, a
scalar path, a generic prime-radix stage).  Each case here
  * feeds standard-normal data from a fixed seed (16-bit sources: rounded first, the reference sees the rounded values),
  * pre-fills every destination with NaN: what the call owns must hold no NaN afterwards, everything else must still be NaN,
  * asserts the exact string fcvsr_last_fft_path() reports, computed from this file's OWN copy of the length table and lane rules - a
    case named "two-stage 160" that fell back to the plan kernels would fail here instead of covering nothing,
  * bounds max|got - ref| by 3e-6 * max|ref| (no floor; 3e-6 is the forward bound of test_hip_ops.test_rfft2_irfft2_vs_torch).  torch's
    own f32 transforms are within 1.8e-7 (forward) / 2.8e-7 (inverse) of float64 at these lengths, so the bound leaves a correct f32
    transform a factor of ten.
Inverse cases feed a spectrum that is NOT Hermitian-consistent and rely on c2r semantics (imaginary parts of the DC / Nyquist columns
are ignored), like torch.fft.irfft2.  B = 2 with line counts that are no multiple of 8 runs the padding workgroups of the rounded-up
grid.

Measured worst max|got - ref| / max|ref| per pass and length on an MI355X, in units of 1e-7 (the bound is 30), over all n of a length.
"rows" columns: test_two_stage_rows / _16bit_source (W = N); "cols": test_two_stage_cols (H = N); "bands": test_bands (H = N; 192,
256 and 240 are its band-by-band fallbacks).  The error is spread evenly everywhere (median / max of |error| >= 0.06 in every case).
     N    rows f32   rows bf16    rows f16    rows inv    cols fwd    cols inv  cols inv+mask    bands
    64       1.9        1.5         1.8         1.5         1.3         1.9         2.0           1.8
    72       2.5        2.5         2.4         1.6         1.5         2.1         2.6           2.2
    80       1.7        1.2         1.4         1.9         1.4         1.6         1.7           1.9
    96       2.4        2.4         2.2         1.6         1.6         2.4         2.1           2.5
   128       1.7        1.4         1.6         1.5         1.4         1.9         1.8           1.9
   144       2.3        2.8         2.5         1.9         1.7         2.4         2.4           2.5
   160       1.8        1.6         1.7         1.5         1.5         1.6         1.9           1.8
   180       2.2        2.2         2.1         1.9         1.8         2.7         2.8           2.6
   192       2.0        2.0         1.9         1.6         1.6         1.8         2.4           2.2
   240       2.5        2.5         2.4         1.9          -           -           -            2.1
   256       2.1        1.9         1.7         1.8         1.8         2.4         2.5           2.5
   320       2.4        2.3         2.3         2.0          -           -           -             -
Plan columns at H = 240 / 320: 1.6 forward, 1.8 inverse.  Layouts (128 x 128 real-first, 64 x 80 three-spectrum): <= 1.7.  Fallbacks at
96 x 160: <= 2.1.  Plan kernels (9 x 176, 26 x 14): <= 2.5.  Training adjoints (128 x 128, 96 x 160), outputs and gradients: <= 1.7
for spec_pack and irfft_pair, <= 2.7 for split_bands.
The inverse checks of test_hip_ops (test_rfft2_irfft2_vs_torch, test_irfft2_bands_equals_band_by_band): <= 2.6.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-6

# ---- this file's own copy of the dispatcher's tables ------------------------------------------------------------------------------
TWO_STAGE = {64: (8, 8), 72: (8, 9), 80: (8, 10), 96: (8, 12), 128: (8, 16), 144: (12, 12), 160: (10, 16), 180: (12, 15),
             192: (12, 16), 240: (15, 16), 256: (16, 16), 320: (16, 20)}
ROW_LENGTHS = sorted(TWO_STAGE)
COL_LENGTHS = [N for N in ROW_LENGTHS if N not in (240, 320)]                 # the 15x16 / 16x20 column butterflies are not built
BAND_LENGTHS = [N for N in COL_LENGTHS if N not in (192, 256)]                # nor the 12x16 / 16x16 ones with the band masks


def lanes2(N, need):
    """Channel lanes of a two-stage workgroup: the largest power of two <= 32 with max(R1, R2) * L <= 512 threads and 8 N L <= 48 KiB
    of LDS, halved while half of it still holds the lanes needed (n / 2 for row passes: two channels per lane; n for column passes)."""
    r1, r2 = TWO_STAGE[N]
    L = 32
    while L > 1 and (max(r1, r2) * L > 512 or 8 * N * L > 49152):
        L //= 2
    while L > 1 and L // 2 >= need:
        L //= 2
    return L


def lanes_plan(N, need):
    """The same for the plan kernels: two ping-pong complex buffers and the twiddles, 16 N L + 8 N bytes, within 64 KiB."""
    L = 32
    while L > 1 and 16 * N * L + 8 * N > 65536:
        L //= 2
    while L > 1 and L // 2 >= need:
        L //= 2
    return L


class Lay:
    """Spectrum layout (floats per pixel, offsets of the imaginary / real parts) and what it allows: 8-byte pair accesses (two-stage
    row kernels) and 16-byte accesses (`vec` of the plan kernels).  torch allocations are at least 256-byte aligned."""

    def __init__(self, ps, im, re):
        self.ps, self.im, self.re = ps, im, re
        self.pair = ps % 2 == 0 and im % 2 == 0 and re % 2 == 0
        self.vec = ps % 4 == 0 and im % 4 == 0 and re % 4 == 0


def packed(n):                                       # [imag | real], the layout of the feature spectra
    return Lay(2 * n, 0, n)


def rows_pass(inverse, W, n, lay, img_pair=True, img_vec=True):
    """img_pair / img_vec: the real image (source or destination view) allows 8-byte channel pairs / 16-byte accesses."""
    name = "irfft_rows" if inverse else "rfft_rows"
    if W in TWO_STAGE and n % 2 == 0 and img_pair and lay.pair:
        return "%s2<%d,%d>/L%d" % ((name,) + TWO_STAGE[W] + (lanes2(W, n // 2),))
    L = lanes_plan(W, (n + 1) // 2)
    return "%s/L%d/vec%d" % (name, L, int(L >= 4 and n % (2 * L) == 0 and img_vec and lay.vec))


def cols_pass(H, n, lay, lengths=COL_LENGTHS, name="fft_cols2"):
    if H in lengths:
        return "%s<%d,%d>/L%d" % ((name,) + TWO_STAGE[H] + (lanes2(H, n),))
    L = lanes_plan(H, n)
    return "fft_cols/L%d/vec%d" % (L, int(L >= 4 and n % L == 0 and lay.vec))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _lib():
    from fcvsr_amd import hip
    return hip, hip.lib()


def _path():
    return _lib()[1].fcvsr_last_fft_path().decode()


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype)


def _close(tag, got, ref, tol=TOL):
    """ref: float64, NaN wherever the call must not write.  Prints the figure (run with -s to collect it) before asserting."""
    got = got.detach().cpu().double()
    own = ~torch.isnan(ref)
    assert not bool(torch.isnan(got[own]).any()), f"{tag}: NaN left in what the call owns"
    assert bool(torch.isnan(got[~own]).all()), f"{tag}: wrote outside what the call owns"
    d = torch.where(own, (got - ref).abs(), torch.zeros_like(ref))
    scale = float(ref[own].abs().max())
    err = float(d.max()) / scale
    at = tuple(int(i) for i in torch.unravel_index(torch.argmax(d), d.shape))
    print(f"FFTERR {tag} {err:.3e} median/max {float(d[own].median()) / max(float(d.max()), 1e-300):.3f} at {at}")
    assert err <= tol, f"{tag}: max|got - ref| = {err:.3e} * max|ref| at {at} (bound {tol:.1e})"


def _spec_buf(g, B, H, Wf, n, lay):
    """Random (not Hermitian-consistent) spectrum in the layout, NaN in the channels that are not part of it; its complex value."""
    buf = _nan(B, H, Wf, lay.ps)
    buf[..., lay.im:lay.im + n] = torch.randn(B, H, Wf, n, generator=g)
    buf[..., lay.re:lay.re + n] = torch.randn(B, H, Wf, n, generator=g)
    z = torch.complex(buf[..., lay.re:lay.re + n].double(), buf[..., lay.im:lay.im + n].double())
    return buf, z


def _spec_ref(X, lay):
    B, H, Wf, n = X.shape
    ref = _nan(B, H, Wf, lay.ps, dtype=torch.float64)
    ref[..., lay.im:lay.im + n] = X.imag
    ref[..., lay.re:lay.re + n] = X.real
    return ref


def _img_ref(y, wide, c0=0):
    B, H, W, n = y.shape
    ref = _nan(B, H, W, wide, dtype=torch.float64)
    ref[..., c0:c0 + n] = y
    return ref


def _rfft2(src_view, B, H, W, n, spec, lay):
    hip, L = _lib()
    v = hip.view(src_view)
    hip.check(L.fcvsr_rfft2(C.byref(v), B, H, W, n, spec.data_ptr(), lay.ps, lay.im, lay.re, hip.stream_ptr()), "rfft2")
    torch.cuda.synchronize()
    return _path()


def _irfft2(spec, lay, B, H, W, n, dst_view, mask=None, work=None):
    hip, L = _lib()
    v = hip.view(dst_view)
    hip.check(L.fcvsr_irfft2(spec.data_ptr(), lay.ps, lay.im, lay.re, B, H, W, n, hip.ptr(mask), hip.ptr(work), C.byref(v),
                             hip.stream_ptr()), "irfft2")
    torch.cuda.synchronize()
    return _path()


def _forward_case(tag, B, H, W, n, lay, dtype=torch.float32, wide=None, c0=0, img_pair=True, img_vec=True):
    """fcvsr_rfft2 of channels c0 : c0 + n of a `wide`-channel tensor into a NaN spectrum buffer; path and values."""
    wide = wide or n
    g = _gen(1, H, W, n, lay.ps, lay.im, wide, c0)
    x = torch.randn(B, H, W, wide, generator=g).to(dtype)                    # what the kernel sees
    ref = _spec_ref(torch.fft.rfft2(x[..., c0:c0 + n].double(), dim=(1, 2)), lay)
    spec = _nan(B, H, W // 2 + 1, lay.ps).cuda()
    xd = x.cuda()
    got = _rfft2(xd[..., c0:c0 + n], B, H, W, n, spec, lay)
    assert got == rows_pass(False, W, n, lay, img_pair, img_vec) + ";" + cols_pass(H, n, lay), got
    _close(tag, spec, ref)


def _inverse_case(tag, B, H, W, n, lay, wide=None, c0=0, img_pair=True, img_vec=True):
    """fcvsr_irfft2 in place (work = NULL) into channels c0 : c0 + n of a `wide`-channel NaN tensor; path and values."""
    wide = wide or n
    Wf = W // 2 + 1
    buf, z = _spec_buf(_gen(2, H, W, n, lay.ps, lay.im, wide, c0), B, H, Wf, n, lay)
    ref = _img_ref(torch.fft.irfft2(z, s=(H, W), dim=(1, 2)), wide, c0)
    spec = buf.cuda()
    dst = _nan(B, H, W, wide).cuda()
    got = _irfft2(spec, lay, B, H, W, n, dst[..., c0:c0 + n])
    assert got == cols_pass(H, n, lay) + ";" + rows_pass(True, W, n, lay, img_pair, img_vec), got
    _close(tag, dst, ref)
    own = ~torch.isnan(buf)
    assert bool(torch.isnan(spec.cpu()[~own]).all()), f"{tag}: the in-place column pass wrote outside the spectrum's channels"


def _short(i):                 # the other, short dimension: 14 = 2 x 7 and 26 = 2 x 13 are plan lengths with a generic prime stage
    return (14, 26)[i % 2]


# ---- a. row instantiations ----------------------------------------------------------------------------------------------------------
ROW_CASES = [(N, n) for N in ROW_LENGTHS for n in (64, 12, 2)] + [(128, 128)]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("N,n", ROW_CASES)
def test_two_stage_rows(N, n, inverse):
    """rfft_rows2_kernel<R1,R2,f32> / irfft_rows2_kernel<R1,R2> at W = N.  n = 12 leaves dead lanes inside a workgroup, n = 2 is one
    lane per workgroup, n = 64 fills L = 32 at N = 192 (50 688 bytes of LDS, the boundary of the lane rule) and takes two channel
    chunks at N = 320, n = 128 at N = 128 takes two chunks at L = 32."""
    H = _short(ROW_LENGTHS.index(N))
    want = ("irfft_rows2" if inverse else "rfft_rows2") + "<%d,%d>/L%d" % (TWO_STAGE[N] + (lanes2(N, n // 2),))
    assert rows_pass(inverse, N, n, packed(n)) == want
    if (N, n) == (192, 64):
        assert want.endswith("/L32") and 8 * N * 32 + 8 * N == 50688
    if (N, n) in ((320, 64), (128, 128)):
        assert 2 * lanes2(N, n // 2) * 2 == n                                 # two chunks of 2 L channels
    tag = f"rows {'inv' if inverse else 'fwd'} N={N} n={n}"
    (_inverse_case if inverse else _forward_case)(tag, 2, H, N, n, packed(n))


# ---- b. 16-bit sources ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", ROW_LENGTHS)
def test_two_stage_rows_16bit_source(N, dtype):
    """rfft_rows2_kernel<R1,R2,bf16|f16>: its own instantiation per length; the reference transforms the rounded values."""
    _forward_case(f"rows16 fwd {str(dtype)[6:]} N={N} n=64", 2, _short(ROW_LENGTHS.index(N)), N, 64, packed(64), dtype=dtype)


# ---- c. column instantiations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 12, 2])
@pytest.mark.parametrize("N", COL_LENGTHS)
def test_two_stage_cols(N, n):
    """fft_cols2_kernel<R1,R2,INV,MASK> at H = N, its three variants: forward, inverse, inverse with a mask in (0, 1] from `spec` into
    `work` (spec must stay bit-unchanged).  The spectrum has 4 spare floats per pixel that no pass may touch."""
    W = _short(COL_LENGTHS.index(N))
    B, Wf = 2, W // 2 + 1
    lay = Lay(2 * n + 4, 0, n)
    want = "fft_cols2<%d,%d>/L%d" % (TWO_STAGE[N] + (lanes2(N, n),))
    assert cols_pass(N, n, lay) == want
    _forward_case(f"cols fwd N={N} n={n}", B, N, W, n, lay)
    _inverse_case(f"cols inv N={N} n={n}", B, N, W, n, lay)
    g = _gen(3, N, W, n)
    buf, z = _spec_buf(g, B, N, Wf, n, lay)
    mask = 1.0 - torch.rand(N, Wf, generator=g)
    ref = torch.fft.irfft2(z * mask.double()[None, :, :, None], s=(N, W), dim=(1, 2))
    spec, work, dst, md = buf.cuda(), _nan(B, N, Wf, lay.ps).cuda(), _nan(B, N, W, n).cuda(), mask.cuda()
    keep = spec.clone()
    got = _irfft2(spec, lay, B, N, W, n, dst, mask=md, work=work)
    assert got == want + ";" + rows_pass(True, W, n, lay), got
    assert torch.equal(spec.view(torch.int32), keep.view(torch.int32)), "the masked inverse changed its input spectrum"
    _close(f"cols invmask N={N} n={n}", dst, ref)
    own = ~torch.isnan(buf)
    wk = work.cpu()
    assert not bool(torch.isnan(wk[own]).any()) and bool(torch.isnan(wk[~own]).all()), "work: spare channels written / owned ones not"


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("N", [240, 320])
def test_cols_240_320_take_the_plan(N, inverse):
    lay = packed(64)
    assert cols_pass(N, 64, lay).startswith("fft_cols/")
    (_inverse_case if inverse else _forward_case)(f"cols plan {'inv' if inverse else 'fwd'} N={N} n=64", 2, N, 14, 64, lay)


# ---- d. band kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 6])
@pytest.mark.parametrize("N", BAND_LENGTHS + [192, 256, 240])
def test_bands(N, n):
    """fcvsr_irfft2_bands with Q = 3 masks: fft_cols2_bands_kernel<R1,R2> for the 8 band lengths, band by band on fft_cols2<..> (with
    a mask) for 192 / 256 and on the plan columns for 240.  Every band against float64, bit-equal to single fcvsr_irfft2 calls, the
    spectrum unchanged; the destinations are n-channel slices of (n + 4)-channel NaN tensors."""
    hip, L = _lib()
    Q, B = 3, 2
    W = _short((BAND_LENGTHS + [192, 256, 240]).index(N))
    Wf = W // 2 + 1
    lay = packed(n)
    g = _gen(4, N, W, n)
    buf, z = _spec_buf(g, B, N, Wf, n, lay)
    masks = 1.0 - torch.rand(Q, N, Wf, generator=g)
    spec, md = buf.cuda(), masks.cuda()
    keep = spec.clone()
    single = _nan(Q, B, N, W, n + 4).cuda()
    work1 = torch.empty(B, N, Wf, lay.ps, device="cuda")
    for q in range(Q):
        _irfft2(spec, lay, B, N, W, n, single[q][..., :n], mask=md[q], work=work1)
    out = _nan(Q, B, N, W, n + 4).cuda()
    work = _nan(Q, B, N, Wf, lay.ps).cuda()
    views = (hip.View * Q)(*[hip.view(out[q][..., :n]) for q in range(Q)])
    hip.check(L.fcvsr_irfft2_bands(spec.data_ptr(), lay.ps, lay.im, lay.re, B, N, W, n, md.data_ptr(), Q, work.data_ptr(), views,
                                   hip.stream_ptr()), "irfft2_bands")
    torch.cuda.synchronize()
    rows = rows_pass(True, W, n, lay, img_vec=(n + 4) % 4 == 0)
    if N in BAND_LENGTHS:
        want = cols_pass(N, n, lay, BAND_LENGTHS, "fft_cols2_bands") + ";" + rows
        assert want.startswith("fft_cols2_bands<%d,%d>/" % TWO_STAGE[N])
    else:
        want = cols_pass(N, n, lay) + ";" + rows
        assert want.startswith("fft_cols/" if N == 240 else "fft_cols2<%d,%d>/" % TWO_STAGE[N])
    assert _path() == want, _path()
    assert torch.equal(spec.view(torch.int32), keep.view(torch.int32)), "the band split changed its input spectrum"
    assert torch.equal(out.view(torch.int32), single.view(torch.int32)), "bands differ from single masked inverse transforms"
    for q in range(Q):
        ref = _img_ref(torch.fft.irfft2(z * masks[q].double()[None, :, :, None], s=(N, W), dim=(1, 2)), n + 4)
        _close(f"bands N={N} n={n} q={q}", out[q], ref)


# ---- e. layouts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_offset_field_layout_128(inverse):
    """The engine's layout for the offset fields: real parts first (re_off = 0, im_off = n, pix_stride = 2 n), n = 12, at the training
    crop 128 x 128; the image is a 12-channel slice of a 16-channel tensor."""
    n = 12
    lay = Lay(2 * n, n, 0)
    assert cols_pass(128, n, lay) == "fft_cols2<8,16>/L16"
    assert rows_pass(inverse, 128, n, lay) == ("irfft_rows2<8,16>/L8" if inverse else "rfft_rows2<8,16>/L8")
    (_inverse_case if inverse else _forward_case)(f"layout re-first {'inv' if inverse else 'fwd'} 128x128 n=12", 2, 128, 128, n, lay,
                                                  wide=16)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_three_spectrum_buffer_64x80(inverse):
    """One spectrum of a buffer that holds three (pix_stride = 6 n, offsets 2 n and 3 n): the other two thirds stay NaN."""
    n = 12
    lay = Lay(6 * n, 2 * n, 3 * n)
    assert rows_pass(inverse, 80, n, lay).startswith(("irfft_rows2" if inverse else "rfft_rows2") + "<8,10>/")
    assert cols_pass(64, n, lay).startswith("fft_cols2<8,8>/")
    (_inverse_case if inverse else _forward_case)(f"layout 3-spectrum {'inv' if inverse else 'fwd'} 64x80 n=12", 2, 64, 80, n, lay)


# ---- f. fallbacks at a two-stage shape ------------------------------------------------------------------------------------------------
FALLBACKS = {
    # an odd channel count has no channel pairs
    "odd_n": dict(n=5, lay=packed(5)),
    # channels 1 : n + 1 of a wider tensor: the pointer is 4 mod 8, no 8-byte pair loads / stores
    "channel_offset": dict(n=8, lay=packed(8), wide=10, c0=1, img_pair=False, img_vec=False),
    # odd spectrum offsets: im_off = 1, re_off = n + 1 in pixels of 2 n + 2 floats
    "odd_im_off": dict(n=8, lay=Lay(18, 1, 9)),
}


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("which", sorted(FALLBACKS))
def test_fallbacks_at_96x160(which, inverse):
    """What keeps a two-stage length off the pair-access ROW kernels: the row pass must report the plan kernel (scalar path) and still
    match.  The column kernels access single floats and have no such condition: H = 96 stays on fft_cols2<8,12>."""
    kw = dict(FALLBACKS[which])
    n, lay = kw.pop("n"), kw.pop("lay")
    want = rows_pass(inverse, 160, n, lay, kw.get("img_pair", True), kw.get("img_vec", True))
    assert want.startswith(("irfft_rows" if inverse else "rfft_rows") + "/") and want.endswith("/vec0"), want
    assert cols_pass(96, n, lay).startswith("fft_cols2<8,12>/")
    (_inverse_case if inverse else _forward_case)(f"fallback {which} {'inv' if inverse else 'fwd'} 96x160 n={n}", 2, 96, 160, n, lay, **kw)


# ---- g. plan-path gaps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("H,W,n,rows,cols", [(9, 176, 64, "rows/L16/vec1", "fft_cols/L32/vec1"),       # two channel chunks in the rows
                                             (26, 14, 64, "rows/L32/vec1", "fft_cols/L32/vec1"),
                                             (26, 14, 6, "rows/L4/vec0", "fft_cols/L8/vec0")])       # channels 6, 7 of the pair absent
def test_plan_kernels(H, W, n, rows, cols, inverse):
    lay = packed(n)
    assert rows_pass(inverse, W, n, lay) == ("irfft_" if inverse else "rfft_") + rows and cols_pass(H, n, lay) == cols
    (_inverse_case if inverse else _forward_case)(f"plan {'inv' if inverse else 'fwd'} {H}x{W} n={n}", 2, H, W, n, lay)


# ---- training adjoints at the lengths training runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,H,W", [(2, 8, 128, 128), (1, 8, 96, 160)])
def test_train_fft_adjoints_at_training_lengths(B, n, H, W):
    """fcvsr_amd.train.fft (spec_pack, irfft_pair, split_bands) forward and backward at the training crop 128 x 128 and at 96 x 160,
    against torch.fft with torch's own autograd, both in float64 on the CPU.  irfft_pair runs n = 2: one lane per row workgroup.
    The path is asserted after each forward only: fcvsr_last_fft_path() is per thread and autograd runs the backward on its own."""
    from fcvsr_amd.engine import band_masks_half
    from fcvsr_amd.train.fft import irfft_pair, spec_pack, split_bands
    g = _gen(5, B, n, H, W)
    Wf = W // 2 + 1
    cl = dict(memory_format=torch.channels_last)
    sz = f"{H}x{W}"
    two = lambda name, N, lanes: "%s<%d,%d>/L%d" % ((name,) + TWO_STAGE[N] + (lanes,))

    x0 = torch.randn(B, n, H, W, generator=g)
    go = torch.randn(B, 2 * n, H, Wf, generator=g)
    x = x0.cuda().contiguous(**cl).requires_grad_(True)
    y = spec_pack(x)
    assert _path() == two("rfft_rows2", W, lanes2(W, n // 2)) + ";" + two("fft_cols2", H, lanes2(H, n)), _path()
    y.backward(go.cuda())
    xr = x0.double().requires_grad_(True)
    X = torch.fft.rfft2(xr)
    yr = torch.cat([X.imag, X.real], 1)
    yr.backward(go.double())
    _close(f"train spec_pack out {sz}", y, yr.detach())
    _close(f"train spec_pack grad {sz}", x.grad, xr.grad)

    o0 = torch.randn(B, 4, H, Wf, generator=g)                                # two complex planes [re0, re1 | im0, im1]
    gy = torch.randn(B, 2, H, W, generator=g)
    o = o0.cuda().contiguous(**cl).requires_grad_(True)
    y = irfft_pair(o, H, W)
    assert lanes2(W, 1) == 1
    assert _path() == two("fft_cols2", H, lanes2(H, 2)) + ";" + two("irfft_rows2", W, 1), _path()
    y.backward(gy.cuda())
    orf = o0.double().requires_grad_(True)
    yr = torch.fft.irfft2(torch.complex(orf[:, :2], orf[:, 2:]), s=(H, W))
    yr.backward(gy.double())
    _close(f"train irfft_pair out {sz}", y, yr.detach())
    _close(f"train irfft_pair grad {sz}", o.grad, orf.grad)

    Q = 4
    M = band_masks_half(Q, H, W).float().cpu()
    gos = [torch.randn(B, n, H, W, generator=g) for _ in range(Q)]
    x = x0.cuda().contiguous(**cl).requires_grad_(True)
    ys = split_bands(x, M.cuda())
    assert _path() == two("fft_cols2_bands", H, lanes2(H, n)) + ";" + two("irfft_rows2", W, lanes2(W, n // 2)), _path()
    sum((a * b.cuda()).sum() for a, b in zip(ys, gos)).backward()
    xr = x0.double().requires_grad_(True)
    X = torch.fft.rfft2(xr)
    yrs = [torch.fft.irfft2(X * M[q].double(), s=(H, W)) for q in range(Q)]
    sum((a * b.double()).sum() for a, b in zip(yrs, gos)).backward()
    for q in range(Q):
        _close(f"train split_bands out{q} {sz}", ys[q], yrs[q].detach())
    _close(f"train split_bands grad {sz}", x.grad, xr.grad)
